"""Random `gmul lM lO lN` calls -- ranks 0..3 on each side, hidden batch on either operand or both, the batch-summed
form, fp32 and fp64 -- against numpy einsum on small integers (bit-exact).  usage: gmul_fuzz.py [cases] [seed]"""
import os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tensor_ops_amd.hipt import HipT
from tools.mismatch_report import same
from tools import poison   # (FUZZ_POISON=1: every case once with +-inf / NaN in the operands, once more clean)
n_cases = int(sys.argv[1]) if len(sys.argv) > 1 else 300
seed = int(sys.argv[2]) if len(sys.argv) > 2 else 0
rng = np.random.default_rng(seed)
Ts = {np.float32: HipT(0), np.float64: HipT(0, dtype=np.float64)}
bad = 0


def poisoned_operands(a, b, ba, bb, B, M, K, N, red):
    """FUZZ_POISON=1: sample 0 of each operand poisoned as a matrix (a: M x K with the contracted indices in order; b: K x N with
    them reversed, as gmul wants them); and, in a batch of five or more that is not summed, one WHOLE other sample of a batched
    operand -- beyond one sample's extent lies the next sample, inside the allocation and inside any buffer descriptor."""
    a, b = a.copy(), b.copy()
    a2 = a.reshape((B if ba else 1, M, K)); b2 = b.reshape((B if bb else 1, K, N))      # (views of the copies)
    a2[0], b2[0] = poison.pair(a2[0], b2[0])
    if B >= 5 and not red:
        s = 1 + poison.integers(B - 1)
        if ba and (not bb or poison.integers(2)):
            a2[s] = poison.draw()
        elif bb:
            b2[s] = poison.draw()
    return a, b


def poison_want(a, b, ba, bb, B, M, K, N, red, os_, dt):
    """the reference of a round through tests/nonfinite_ref.py: sample by sample, the summed form as ONE contraction over (z, k)"""
    a2 = a.reshape((B if ba else 1, M, K)).astype(np.float64)
    kshape = tuple(os_[::-1])
    b2 = b.reshape((B if bb else 1,) + kshape + (N,))
    b2 = b2.transpose((0,) + tuple(range(len(kshape), 0, -1)) + (len(kshape) + 1,)).reshape(-1, K, N).astype(np.float64)   # (k in a's order)
    if red:
        return poison.reference(np.concatenate(list(a2), axis=1), np.concatenate(list(b2), axis=0)).astype(dt)
    nb = B if (ba or bb) else 1
    return np.stack([poison.reference(a2[z if ba else 0], b2[z if bb else 0]) for z in range(nb)]).astype(dt)


for case in range(n_cases):
    dt = np.float32 if rng.random() < 0.7 else np.float64
    T = Ts[dt]
    lm, lo, ln = int(rng.integers(0, 4)), int(rng.integers(0, 4)), int(rng.integers(0, 4))
    if lm + lo > 4 or lo + ln > 4:
        continue
    big = rng.random() < 0.2
    d = lambda: int(rng.integers(1, 40 if big else 7))
    ms, os_, ns = [d() for _ in range(lm)], [d() for _ in range(lo)], [d() for _ in range(ln)]
    ba, bb = bool(rng.integers(2)), bool(rng.integers(2))
    B = int(rng.choice([1, 2, 5, 33]))
    red = (ba and bb) and rng.random() < 0.4
    a0 = rng.integers(-2, 3, ([B] if ba else []) + ms + os_).astype(dt)
    b0 = rng.integers(-2, 3, ([B] if bb else []) + os_[::-1] + ns).astype(dt)
    L = "abcdefghijklmnop"
    mi, oi, ni = L[:lm], L[lm:lm + lo], L[lm + lo:lm + lo + ln]
    sa, sb = ("z" if ba else "") + mi + oi, ("z" if bb else "") + oi[::-1] + ni
    so = ("" if red or not (ba or bb) else "z") + mi + ni
    M_, K_, N_ = int(np.prod(ms, dtype=np.int64)), int(np.prod(os_, dtype=np.int64)), int(np.prod(ns, dtype=np.int64))
    for a, b in ([poisoned_operands(a0, b0, ba, bb, B, M_, K_, N_, red), (a0, b0)] if poison.ON else [(a0, b0)]):
        if poison.ON:
            want = poison_want(a, b, ba, bb, B, M_, K_, N_, red, os_, dt)
            poison.count(want.reshape(-1, N_), M_, N_, a is not a0)
            want = want.reshape(([B] if (ba or bb) and not red else []) + ms + ns)
        else:
            want = np.einsum("%s,%s->%s" % (sa, sb, so), a.astype(np.float64), b.astype(np.float64)).astype(dt)
        A, Bt = T.put(a, batched=ba), T.put(b, batched=bb)
        try:
            got = (T.gmul_batch_sum if red else T.gmul)(lm, lo, ln, A, Bt).numpy()
        except Exception as e:  # noqa: BLE001
            bad += 1
            print("ERROR", case, dt.__name__, (lm, lo, ln), ms, os_, ns, "batch", ba, bb, B, "red", red, repr(e)[:200])
            continue
        got = np.asarray(got).reshape(want.shape) if got.size == want.size else got
        if not (poison.same(got, want) if poison.ON else same(got, want, tool='gmul_fuzz', case=case, dtype=dt.__name__, lm=lm, lo=lo, ln=ln, ms=ms, os=os_, ns=ns, ba=ba, bb=bb, B=B, red=red)):
            bad += 1
            print("MISMATCH", case, dt.__name__, (lm, lo, ln), ms, os_, ns, "batch", ba, bb, B, "red", red, got.shape, want.shape)
poison.report("gmul_fuzz")
print("cases", n_cases, "mismatches", bad)
