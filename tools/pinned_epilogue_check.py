"""The pinned 256x256 body's fused way out (bias, bias + logistic) on large layers: a recorded `W x + b` (batched matVec +
sumT), alone and under logistic, against numpy -- integers, so the pre-activation is exact.  Full tiles and edge tiles."""
import os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tensor_ops_amd import hipt
from tensor_ops_amd.hipt import HipT
from tools.mismatch_report import same
from tools import poison   # (FUZZ_POISON=1: every case once with +-inf / NaN in the operands, once more clean)
T = HipT(0)
rng = np.random.default_rng(9)
bad = 0
for (M, K, N) in ((4096, 64, 4096), (4096, 272, 4096), (4000, 288, 4000), (4352, 1024, 4352), (8192, 48, 2048)):
    W0 = rng.integers(-2, 3, (N, K)).astype(np.float32); X0 = rng.integers(-2, 3, (M, K)).astype(np.float32)
    b = rng.integers(-3, 4, N).astype(np.float32)
    for X, Wt in poison.rounds(X0, W0.T):
        W = np.ascontiguousarray(Wt.T)
        want = poison.want_product(X, Wt, np.float64, bias=b) if poison.ON else X.astype(np.float64) @ W.T.astype(np.float64) + b
        dW, dX, db = T.put(W), T.put(X, batched=True), T.put(b)
        l0 = T.stats()["launches"]
        with T.memo():
            z = T.force(T.sumT([T.matVec(dW, dX), db], (N,)))
        nl = T.stats()["launches"] - l0
        ok = poison.same(z.numpy().reshape(M, N), want.astype(np.float32)) if poison.ON else same(z.numpy(), want.astype(np.float32), tool='pinned_epilogue_check', M=M, K=K, N=N)
        l0 = T.stats()["launches"]
        with T.memo():
            h = T.force(T.liftT(hipt.logistic_closure, [T.sumT([T.matVec(dW, dX), db], (N,))], key="pe-logistic"))
        nl2 = T.stats()["launches"] - l0
        if poison.ON:
            ref = poison.logistic(want)
            ok = ok and poison.close(h.numpy().reshape(M, N), ref, 2e-6)
            err = float(np.nanmax(np.abs(h.numpy().reshape(M, N) - ref)))
        else:
            err = float(np.max(np.abs(h.numpy() - 1 / (1 + np.exp(-want)))))
            ok = ok and err < 2e-6
        print((M, K, N), "launches", nl, nl2, "logistic err %.2e" % err, "ok" if ok else "MISMATCH")
        bad += not ok
        del dW, dX, db, z, h
poison.report("pinned_epilogue_check")
print("mismatches", bad)
if poison.ON:
    sys.exit(0)   # (the timing below belongs to the plain run)
# what the fused way out costs next to the plain product (4096^3, steady state)
M = K = N = 4096
W = T.genRand((N, K), "uniform", -1, 1, 1)
X = T.put(rng.uniform(-1, 1, (M, K)).astype(np.float32), batched=True)
b = T.put(rng.uniform(-1, 1, N).astype(np.float32))


def timed(fn, n=60, warm=80):
    for _ in range(warm): fn()
    T.sync(); T.timer_start()
    for _ in range(n): fn()
    return T.timer_stop() / n


def plain():
    with T.memo():
        T.force(T.matVec(W, X))


def fused():
    with T.memo():
        T.force(T.liftT(hipt.logistic_closure, [T.sumT([T.matVec(W, X), b], (N,))], key="pe-logistic"))


print("4096^3 batched matVec            %.4f ms" % timed(plain))
print("4096^3 logistic(matVec + bias)   %.4f ms (one launch)" % timed(fused))
