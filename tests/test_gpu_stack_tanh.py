"""tanh hidden layers (`genNet ws (actMap tanh) out`, hidden_act = TO_ACT_TANH) through the one-call ffLayer stack entries:
to_fflayer_stack_grad / _sgd, _online_sgd, _infer and _induce.

Checked against the numpy restatement of tests/act_numpy.py (held to the oracle at 1e-12 by tests/test_act_numpy_ref.py) on
the smallest shapes that reach each code path: the loss head with the fused tail (both heads), a head wider than 16 (no
fused head), the one-sample rank-1 route, the step's big GEMM kernels at 784-256-10 / 1024, a deeper stack; the persistent
online kernel at G = 1 and G = 32; the infer head narrow and wide, the fp64 hidden layer whose GEMM has no fused epilogue,
infinities and NaN; both induce routes.  Tolerances are those of the logistic tests of the same entries."""
import ctypes as C

import numpy as np
import pytest

import act_numpy as AN

pytestmark = pytest.mark.gpu
DTS = [np.float32, np.float64]
RTOL = {np.float32: 1e-5, np.float64: 1e-11}      # relative, grad / sgd / online (tests/test_gpu_online.py)
ATOL = {np.float32: 1e-5, np.float64: 1e-12}      # absolute, infer / induce (tests/test_gpu_infer.py, test_gpu_induce.py)
LOSS = {"softmax": "crossEntropy", "logistic": "squaredError"}


@pytest.fixture(scope="module")
def Ts():
    from tensor_ops_amd.hipt import HipT
    return {np.float32: HipT(0, np.float32), np.float64: HipT(0, np.float64)}


def rel_err(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    return np.linalg.norm((got - want).ravel()) / max(np.linalg.norm(want.ravel()), 1e-300)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def problem(sizes, B, dt, seed, out_act="softmax"):
    """weights N(0, 1 / fan_in), rows in [-1, 1], soft targets (one-hot is the special case the kernels do not need)"""
    rng = np.random.default_rng(seed)
    ws = [((rng.standard_normal((o, i)) / np.sqrt(i)).astype(dt), (0.5 * rng.standard_normal(o)).astype(dt))
          for i, o in zip(sizes[:-1], sizes[1:])]
    X = rng.uniform(-1, 1, (B, sizes[0])).astype(dt)
    Y = rng.uniform(0.05, 0.95, (B, sizes[-1])).astype(dt)
    if out_act == "softmax":
        Y = (Y / Y.sum(axis=1, keepdims=True)).astype(dt)
    return ws, X, Y


def put_net(T, ws):
    return [T.put(w) for w, _ in ws], [T.put(b) for _, b in ws]


def ident(v):
    if isinstance(v, list):
        return "-".join(map(str, v))
    return getattr(v, "__name__", str(v))


# ---- grad / sgd -----------------------------------------------------------------------------------------------------------
# (sizes, B, out_act, dtypes)
STEP = [
    ([30, 14, 6], 64, "softmax", DTS),          # loss head + tail fused
    ([30, 14, 6], 64, "logistic", DTS),         # the other head, same launch
    ([40, 28, 24], 64, "softmax", DTS),         # head wider than 16: no fused head
    ([30, 14, 6], 1, "softmax", DTS),           # one sample: the rank-1 route
    ([784, 256, 10], 1024, "softmax", [np.float32]),   # the step's big forward and the weight-gradient pair
    ([20, 16, 12, 8, 4], 32, "softmax", DTS),   # a deeper stack
]
STEP = [(s, B, o, dt) for s, B, o, dts in STEP for dt in dts]


@pytest.mark.parametrize("sizes,B,out_act,dt", STEP, ids=ident)
def test_grad_and_sgd(Ts, sizes, B, out_act, dt):
    T = Ts[dt]
    ws, X, Y = problem(sizes, B, dt, 0x7a + B + len(sizes), out_act)
    want_g, want_l, _ = AN.grads(ws, X, Y, "tanh", out_act)
    W, b = put_net(T, ws)
    x, y = T.put(X, batched=True), T.put(Y, batched=True)
    gW, gB, losses = T.stack_grad(W, b, x, y, out_act, LOSS[out_act], hidden_act="tanh", want_losses=True)
    errs = [rel_err(g.numpy(), w) for g, (w, _) in zip(gW, want_g)] + [rel_err(g.numpy(), w) for g, (_, w) in zip(gB, want_g)]
    lerr = rel_err(losses.numpy(), want_l)
    print("grad", errs, "losses", lerr)
    assert max(errs) < RTOL[dt] and lerr < RTOL[dt]
    for (w, bb), dw, db in zip(ws, W, b):       # the gradients' call leaves the parameters alone
        assert np.array_equal(dw.numpy(), w) and np.array_equal(db.numpy(), bb)
    rate = 0.05
    T.stack_sgd(W, b, x, y, rate, out_act, LOSS[out_act], hidden_act="tanh")
    want = AN.sgd(ws, X, Y, rate, "tanh", out_act)
    errs = [max(rel_err(dw.numpy(), w), rel_err(db.numpy(), bb)) for (w, bb), dw, db in zip(want, W, b)]
    print("sgd", errs)
    assert max(errs) < RTOL[dt]
    assert not np.array_equal(W[0].numpy(), ws[0][0])   # ... and the step moved them


@pytest.mark.parametrize("sizes,B", [([784, 256, 10], 1024), ([30, 14, 6], 64)], ids=ident)
def test_a_tanh_step_takes_the_logistic_steps_launches(Ts, sizes, B):
    T = Ts[np.float32]
    ws, X, Y = problem(sizes, B, np.float32, 5)
    x, y = T.put(X, batched=True), T.put(Y, batched=True)

    def launches(hidden, sgd):
        W, b = put_net(T, ws)
        call = (lambda: T.stack_sgd(W, b, x, y, 1e-3, hidden_act=hidden)) if sgd else (lambda: T.stack_grad(W, b, x, y, hidden_act=hidden))
        call()                                   # (anything a first call does once per process is not counted)
        T.sync()
        n0 = T.stats()["launches"]
        call()
        T.sync()
        return T.stats()["launches"] - n0

    for sgd in (False, True):
        lg, th = launches("logistic", sgd), launches("tanh", sgd)
        assert lg == th and lg >= 2, (sgd, lg, th)


# ---- online ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS, ids=ident)
@pytest.mark.parametrize("sizes,out_act,n,rate", [([2, 12, 8, 1], "logistic", 100, 0.5), ([30, 14, 6], "softmax", 120, 0.1),
                                                  ([784, 300, 100, 10], "softmax", 64, 0.02)], ids=ident)   # the last: G = 32
def test_online_is_the_per_sample_loop(Ts, sizes, out_act, n, rate, dt):
    from tensor_ops_amd import capi
    T = Ts[dt]
    ws, X, Y = problem(sizes, n + 9, dt, 0x0b + n, out_act)
    order = np.random.default_rng(n).permutation(len(X))[:n]
    want = AN.online(ws, X, Y, order, rate, "tanh", out_act)
    W, b = put_net(T, ws)
    idx = (C.c_int64 * n)(*[int(v) for v in order])
    dX, dY = T.put(X, batched=True), T.put(Y, batched=True)
    st = capi.lib().to_fflayer_stack_online_sgd(len(ws), (capi.c_tensor * len(ws))(*[t.h for t in W]),
                                                (capi.c_tensor * len(ws))(*[t.h for t in b]), 3, 2 if out_act == "softmax" else 0,
                                                1 if out_act == "softmax" else 0, dX.h, dY.h, n, idx, rate)
    assert st == 0, capi.lib().to_last_error()    # not TO_ERR_UNSUPPORTED
    errs = [max(rel_err(dw.numpy(), w), rel_err(db.numpy(), bb)) for (w, bb), dw, db in zip(want, W, b)]
    print("online", errs)
    assert max(errs) < RTOL[dt]
    # the Python wrapper, rows in their own order
    W2, b2 = put_net(T, ws)
    T.stack_online_sgd(W2, b2, dX, dY, n, rate, out_act=out_act, loss=LOSS[out_act],
                       hidden_act="tanh")
    want = AN.online(ws, X, Y, range(n), rate, "tanh", out_act)
    assert rel_err(W2[0].numpy(), want[0][0]) < RTOL[dt]


# ---- infer ----------------------------------------------------------------------------------------------------------------
def infer(T, W, b, X, out_act="softmax", **kw):
    out, cls, conf = T.infer_stack(W, b, T.put(X, batched=True), out_act=out_act, want_out=True, hidden_act="tanh", **kw)
    return out.numpy(), cls, conf


@pytest.mark.parametrize("dt", DTS, ids=ident)
@pytest.mark.parametrize("sizes,B", [([30, 14, 6], 37), ([30, 14, 40], 5)], ids=ident)   # narrow head; head wider than 32
def test_infer(Ts, sizes, B, dt):
    T = Ts[dt]
    for out_act in ("softmax", "logistic"):
        ws, X, Y = problem(sizes, B, dt, 0x1f + B, out_act)
        W, b = put_net(T, ws)
        out, cls, conf = infer(T, W, b, X, out_act, y=T.put(Y, batched=True))
        _, want = AN.forward(ws, X, "tanh", out_act)
        err = np.abs(out - want).max()
        print("infer", out_act, err)
        assert err <= ATOL[dt]
        assert np.array_equal(cls, T.arg_max(T.put(out, batched=True)))
        wc = np.zeros((sizes[-1], sizes[-1]), np.int64)
        np.add.at(wc, (cls, Y.argmax(axis=1)), 1)
        assert np.array_equal(conf, wc) and conf.sum() == B
        # a row alone and inside the batch: identical bits
        for r in (0, B - 1):
            alone, ca, _ = infer(T, W, b, X[r:r + 1], out_act)
            assert np.array_equal(bits(alone[0]), bits(out[r])) and ca[0] == cls[r]


def test_infer_fp64_hidden_layer_without_a_fused_epilogue(Ts):
    """fp64, [5, 70, 6] over 6337 rows: the hidden GEMM is 6337 x 70 x 5 -- 100 x 2 = 200 tiles of 64 x 64, the first count
    that is neither gemm_small_applicable (tiles64 < 200) nor taken as `t64 < 200 && gemm_small_can`; K = 5 < 64 keeps it off
    the wave-split fp64 kernel and no extent is 1 (gemv): the tiled fp64 kernel, alpha / beta only, then bias_act_kernel.
    6336 rows (198 tiles) take the fused epilogue; both must be the same function."""
    T = Ts[np.float64]
    ws, X, _ = problem([5, 70, 6], 6337, np.float64, 0x64)
    W, b = put_net(T, ws)
    n0 = T.stats()["launches"]
    out, cls, _ = infer(T, W, b, X)
    n1 = T.stats()["launches"]
    fused, _, _ = infer(T, W, b, X[:6336])
    n2 = T.stats()["launches"]
    assert (n1 - n0) - (n2 - n1) == 1            # the elementwise launch behind the plain GEMM
    _, want = AN.forward(ws, X, "tanh", "softmax")
    assert np.abs(out - want).max() <= ATOL[np.float64]
    assert np.abs(fused - want[:6336]).max() <= ATOL[np.float64]
    assert np.array_equal(cls, want.argmax(axis=1))


@pytest.mark.parametrize("dt", DTS, ids=ident)
def test_infer_infinities_and_nan(Ts, dt):
    """a row of x holding +inf and -inf drives every hidden unit to exactly +1 or -1 (the signs of W_1's first two columns
    are opposite in every row, so no inf - inf arises); a NaN row is NaN throughout and leaves its neighbours' bits alone"""
    T = Ts[dt]
    ws, X, _ = problem([30, 14, 6], 37, dt, 0x1f)
    ws[0][0][:, 1] = -np.sign(ws[0][0][:, 0]) * np.abs(ws[0][0][:, 1])
    W, b = put_net(T, ws)
    clean, _, _ = infer(T, W, b, X)
    Xi = X.copy()
    Xi[5, 0], Xi[5, 1] = np.inf, -np.inf
    Xi[9, 3] = np.nan
    out, cls, _ = infer(T, W, b, Xi)
    h = np.sign(ws[0][0][:, 0]).astype(np.float64)   # tanh(+-inf)
    z = ws[1][0].astype(np.float64) @ h + ws[1][1]
    assert np.abs(out[5] - AN.softmax(z)).max() <= ATOL[dt]
    assert np.isnan(out[9]).all()
    rest = np.setdiff1d(np.arange(37), [5, 9])
    assert np.array_equal(bits(out[rest]), bits(clean[rest]))
    assert np.array_equal(cls, T.arg_max(T.put(out, batched=True)))


# ---- induce ---------------------------------------------------------------------------------------------------------------
def induce(T, W, b, X, Y, rate, iters, out_act):
    out, g, ls = T.induce_stack(W, b, T.put(X, batched=True), T.put(Y, batched=True), rate, iters, out_act=out_act,
                                loss=LOSS[out_act], want_gx=True, want_losses=True, hidden_act="tanh")
    return out.numpy(), g.numpy(), ls.numpy()


INDUCE = [([30, 14, 6], 5, 0, np.float32), ([30, 14, 6], 5, 0, np.float64), ([30, 14, 6], 5, 2, np.float32),
          ([30, 14, 6], 5, 2, np.float64), ([784, 300, 100, 10], 2, 2, np.float32)]   # the last: G = 32


@pytest.mark.parametrize("sizes,B,mode,dt", INDUCE, ids=ident)
def test_induce(Ts, sizes, B, mode, dt):
    T = Ts[dt]
    prev = T.induce_persistent(mode)
    try:
        for out_act in ("softmax", "logistic"):
            ws, X, Y = problem(sizes, B, dt, 0x1d + B, out_act)
            W, b = put_net(T, ws)
            p0, q0 = T.induce_stats()
            out, gx, ls = induce(T, W, b, X, Y, 0.3, 3, out_act)
            p1, q1 = T.induce_stats()
            assert (p1 - p0) + (q1 - q0) == 1
            print("induce route", sizes, dt.__name__, "mode", mode, "persistent" if p1 > p0 else "per iteration")
            if mode == 0:
                assert q1 - q0 == 1              # per iteration
            elif len(sizes) == 3:
                assert p1 - p0 == 1              # fits one workgroup: persistent when forced
            # (784-300-100-10 needs 32 workgroups a row on one XCD; where the device does not place them so it runs per
            #  iteration under mode 2 as well -- its results are checked all the same)
            want, wg, wl = AN.induce(ws, X, Y, 0.3, 3, "tanh", out_act)
            errs = (np.abs(out - want).max(), np.abs(gx - wg).max(), np.abs(ls - wl).max() / max(1.0, wl.max()))
            print("induce", out_act, mode, errs)
            assert max(errs) <= ATOL[dt]
            assert np.abs(want - X).max() >= 1e-3    # the steps moved x far beyond the tolerance
            # iters 2, then iters 1 on the result, is iters 3 bit for bit
            mid, _, l2 = induce(T, W, b, X, Y, 0.3, 2, out_act)
            end, g1, l1 = induce(T, W, b, mid, Y, 0.3, 1, out_act)
            assert np.array_equal(bits(end), bits(out)) and np.array_equal(bits(g1), bits(gx))
            assert np.array_equal(bits(np.concatenate([l2, l1], axis=1)), bits(ls))
    finally:
        T.induce_persistent(prev)
