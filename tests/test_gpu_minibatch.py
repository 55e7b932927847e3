"""to_fflayer_stack_minibatch_sgd: minibatch SGD over a resident data set in one call.

The yardstick for bits is the host loop made of entry points that were there before it: `batch_gather` (or `batch_slice`
when there is no index table) on X and Y, then `stack_sgd`, per step; equality is equality of the uint32 / uint64 views of
the parameters and of the per-row losses (the loop's per-step losses concatenated).  Shapes are the smallest that reach each
path of the staging launch: [5, 4, 3] has 20- and 12-byte fp32 rows (element pieces), [8, 6, 4] 16-byte multiples (wide
pieces for X, and for Y in fp32), [784, 32, 10] wide X rows next to narrow Y rows in one launch; M = 1 is the rank-1 step,
7 an odd batch, 16 and 128 the batched kernels; n_idx = 3 M has no tail, 3 M + max(1, M // 2) a short one.  Against numpy
(tests/minibatch_numpy.py) the tolerance is RTOL of tests/test_gpu_stack_tanh.py."""
import ctypes as C

import numpy as np
import pytest

import minibatch_numpy as MN

pytestmark = pytest.mark.gpu
DTS = [np.float32, np.float64]
RTOL = {np.float32: 1e-5, np.float64: 1e-11}      # tests/test_gpu_stack_tanh.py: grad / sgd / online
LOSS = {"softmax": "crossEntropy", "logistic": "squaredError"}
HID = {"logistic": 0, "tanh": 3}
OUT = {"softmax": 2, "logistic": 0, "tanh": 3}
LOSS_ID = {"squaredError": 0, "crossEntropy": 1}
OK, ARG, SHAPE, STATE, UNSUPPORTED = 0, 1, 2, 4, 5
N_ROWS = 150


@pytest.fixture(scope="module")
def Ts():
    from tensor_ops_amd.hipt import HipT
    return {np.float32: HipT(0, np.float32), np.float64: HipT(0, np.float64)}


def ident(v):
    if isinstance(v, list):
        return "-".join(map(str, v))
    return getattr(v, "__name__", str(v))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def rel_err(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    return np.linalg.norm((got - want).ravel()) / max(np.linalg.norm(want.ravel()), 1e-300)


def problem(sizes, N, dt, seed, out_act="softmax"):
    rng = np.random.default_rng(seed)
    ws = [((rng.standard_normal((o, i)) / np.sqrt(i)).astype(dt), (0.5 * rng.standard_normal(o)).astype(dt))
          for i, o in zip(sizes[:-1], sizes[1:])]
    X = rng.uniform(-1, 1, (N, sizes[0])).astype(dt)
    Y = rng.uniform(0.05, 0.95, (N, sizes[-1])).astype(dt)
    if out_act == "softmax":
        Y = (Y / Y.sum(axis=1, keepdims=True)).astype(dt)
    return ws, X, Y


def put_net(T, ws):
    return [T.put(w) for w, _ in ws], [T.put(b) for _, b in ws]


def params(W, b):
    return [t.numpy() for t in W] + [t.numpy() for t in b]


def draw_idx(N, n_idx, M, seed):
    """with repeats; holds row 0, row N - 1 and (M >= 2) the same row twice inside the second minibatch"""
    idx = np.random.default_rng(seed).integers(0, N, n_idx).astype(np.int64)
    idx[0], idx[-1] = 0, N - 1
    if M >= 2:
        idx[M + 1] = idx[M]
    return idx


def host_loop(T, W, b, x, y, idx, n, M, rate, out_act, hidden):
    """the yardstick: per step gather (idx) or slice (idx None) X and Y, then stack_sgd.  Returns (losses [n], the launch
    count of the stack_sgd calls alone)."""
    losses, launches = [], 0
    for s, e in MN.batches(n, M):
        if idx is None:
            bx, by = T.batch_slice(x, s, e - s), T.batch_slice(y, s, e - s)
        else:
            bx, by = T.batch_gather(x, idx[s:e]), T.batch_gather(y, idx[s:e])
        n0 = T.stats()["launches"]
        ls = T.stack_sgd(W, b, bx, by, rate, out_act, LOSS[out_act], hidden_act=hidden, want_losses=True)
        launches += T.stats()["launches"] - n0
        losses.append(ls.numpy())
    return np.concatenate(losses), launches


def one_call(T, W, b, x, y, idx, n, M, rate, out_act, hidden):
    """(losses [n], the call's launch count)"""
    n0 = T.stats()["launches"]
    ls = T.stack_minibatch_sgd(W, b, x, y, rate, M, idx=idx, n=n, out_act=out_act, loss=LOSS[out_act], hidden_act=hidden,
                               want_losses=True)
    return ls.numpy(), T.stats()["launches"] - n0


def assert_same_training(T, ws, x, y, idx, n, M, out_act, hidden, rate=0.05):
    W1, b1 = put_net(T, ws)
    want_l, step_launches = host_loop(T, W1, b1, x, y, idx, n, M, rate, out_act, hidden)
    W2, b2 = put_net(T, ws)
    got_l, launches = one_call(T, W2, b2, x, y, idx, n, M, rate, out_act, hidden)
    for got, want, w0 in zip(params(W2, b2), params(W1, b1), [w for w, _ in ws] + [bb for _, bb in ws]):
        assert same_bits(got, want), (M, n)
        assert not np.array_equal(got, w0)          # ... and the steps moved every parameter
    assert same_bits(got_l, want_l), (M, n)
    return step_launches, launches


# ---- 1. bit equality with the host loop -------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS, ids=ident)
@pytest.mark.parametrize("hidden", ["logistic", "tanh"])
@pytest.mark.parametrize("out_act", ["softmax", "logistic"])
@pytest.mark.parametrize("sizes", [[5, 4, 3], [8, 6, 4], [784, 32, 10]], ids=ident)
def test_bit_equal_to_the_host_loop(Ts, sizes, out_act, hidden, dt):
    T = Ts[dt]
    ws, X, Y = problem(sizes, N_ROWS, dt, 0x6d + sizes[0], out_act)
    x, y = T.put(X, batched=True), T.put(Y, batched=True)
    for M in (1, 7, 16, 128):
        for n_idx in (3 * M, 3 * M + max(1, M // 2)):
            idx = draw_idx(N_ROWS, n_idx, M, 7 * M + n_idx)
            steps, launches = assert_same_training(T, ws, x, y, idx, n_idx, M, out_act, hidden)
            assert launches == steps + 1            # one staging launch: everything fits one chunk at the default bound
    assert same_bits(x.numpy(), X) and same_bits(y.numpy(), Y)


# ---- 2. no index table: views, no staging ----------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS, ids=ident)
@pytest.mark.parametrize("sizes,M,n", [([5, 4, 3], 7, 45), ([784, 32, 10], 16, 48), ([8, 6, 4], 1, 3)], ids=ident)
def test_without_indices_the_steps_run_on_views(Ts, sizes, M, n, dt):
    T = Ts[dt]
    ws, X, Y = problem(sizes, N_ROWS, dt, 0x21)
    x, y = T.put(X, batched=True), T.put(Y, batched=True)
    steps, launches = assert_same_training(T, ws, x, y, None, n, M, "softmax", "logistic")
    assert launches == steps and steps >= len(MN.batches(n, M))    # zero staging launches
    # n left out: every row
    W, b = put_net(T, ws)
    ls = T.stack_minibatch_sgd(W, b, x, y, 0.05, 64, want_losses=True)
    W2, b2 = put_net(T, ws)
    want_l, _ = host_loop(T, W2, b2, x, y, None, N_ROWS, 64, 0.05, "softmax", "logistic")
    assert same_bits(ls.numpy(), want_l) and all(same_bits(p, q) for p, q in zip(params(W, b), params(W2, b2)))


# ---- 3. reconstruction ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS, ids=ident)
def test_reconstruction_is_the_call_with_a_copy_of_x(Ts, dt):
    T = Ts[dt]
    ws, X, _ = problem([8, 5, 8], 40, dt, 0x33, "logistic")
    X = (0.5 * X + 0.5).astype(dt)
    x, x2 = T.put(X, batched=True), T.put(X.copy(), batched=True)
    for idx, n in ((draw_idx(40, 25, 6, 3), 25), (None, 25)):
        W1, b1 = put_net(T, ws)
        l1, k1 = one_call(T, W1, b1, x, None, idx, n, 6, 0.1, "logistic", "logistic")
        W2, b2 = put_net(T, ws)
        l2, k2 = one_call(T, W2, b2, x, x2, idx, n, 6, 0.1, "logistic", "logistic")
        assert same_bits(l1, l2) and all(same_bits(p, q) for p, q in zip(params(W1, b1), params(W2, b2)))
        assert k1 == k2                             # no second launch for the targets either way
        assert not np.array_equal(W1[0].numpy(), ws[0][0])
    assert same_bits(x.numpy(), X)


def test_reconstruction_needs_an_output_of_xs_width(Ts):
    from tensor_ops_amd import capi
    T = Ts[np.float32]
    ws, X, _ = problem([8, 5, 3], 40, np.float32, 0x34, "logistic")
    W, b = put_net(T, ws)
    with pytest.raises(capi.TensorOpsError) as e:
        T.stack_minibatch_sgd(W, b, T.put(X, batched=True), None, 0.1, 6, out_act="logistic", loss="squaredError")
    assert e.value.code == SHAPE
    assert all(same_bits(p, q) for p, q in zip(params(W, b), [w for w, _ in ws] + [bb for _, bb in ws]))


# ---- 4. chunking ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS, ids=ident)
def test_chunks_follow_the_stage_bound(Ts, dt):
    T = Ts[dt]
    sizes, M, n_idx = [8, 6, 4], 4, 20                  # five steps
    ws, X, Y = problem(sizes, 50, dt, 0x44)
    x, y = T.put(X, batched=True), T.put(Y, batched=True)
    idx = draw_idx(50, n_idx, M, 9)
    one_step = M * (sizes[0] + sizes[-1]) * np.dtype(dt).itemsize    # the gathered X and Y rows of a step (16-byte multiples)
    W0, b0 = put_net(T, ws)
    _, steps = host_loop(T, W0, b0, x, y, idx, n_idx, M, 0.05, "softmax", "logistic")
    default = T.minibatch_stage_bytes(0)
    try:
        assert default == 32 << 20
        W, b = put_net(T, ws)
        want_l, launches = one_call(T, W, b, x, y, idx, n_idx, M, 0.05, "softmax", "logistic")
        want = params(W, b)
        assert launches == steps + 1
        assert all(same_bits(p, q) for p, q in zip(want, params(W0, b0)))
        before = default
        for bound, chunks in ((one_step, 5), (2 * one_step, 3), (1, 5)):
            assert T.minibatch_stage_bytes(bound) == before     # the setter returns the previous value
            before = bound
            W, b = put_net(T, ws)
            got_l, launches = one_call(T, W, b, x, y, idx, n_idx, M, 0.05, "softmax", "logistic")
            assert launches == steps + chunks, (bound, launches, steps)
            assert same_bits(got_l, want_l) and all(same_bits(p, q) for p, q in zip(params(W, b), want)), bound
        assert T.minibatch_stage_bytes(0) == 1 and T.minibatch_stage_bytes(0) == default    # 0 restores the default
        with pytest.raises(Exception):
            T.minibatch_stage_bytes(-1)
    finally:
        T.minibatch_stage_bytes(default)


# ---- 5. a permutation beyond the pinned ring -------------------------------------------------------------------------------
def test_index_table_larger_than_the_ring(Ts):
    T = Ts[np.float32]
    ws, X, Y = problem([5, 4, 3], 600, np.float32, 0x55)
    x, y = T.put(X, batched=True), T.put(Y, batched=True)
    n_idx = 8200                                        # 65,600 bytes of indices: past the ring's 64 KiB
    idx = draw_idx(600, n_idx, 128, 5)
    assert_same_training(T, ws, x, y, idx, n_idx, 128, "softmax", "logistic", rate=1e-3)


# ---- 6. against numpy -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS, ids=ident)
@pytest.mark.parametrize("hidden", ["logistic", "tanh"])
@pytest.mark.parametrize("sizes,M", [([784, 32, 10], 16), ([5, 4, 3], 7)], ids=ident)
def test_against_numpy(Ts, sizes, M, hidden, dt):
    T = Ts[dt]
    n_idx = 3 * M + M // 2                              # four steps, the last one short
    for out_act in ("softmax", "logistic"):
        ws, X, Y = problem(sizes, N_ROWS, dt, 0x66 + M, out_act)
        idx = draw_idx(N_ROWS, n_idx, M, 11)
        want, want_l = MN.minibatch_sgd(ws, X, Y, idx, M, 0.05, hidden, out_act)
        W, b = put_net(T, ws)
        got_l, _ = one_call(T, W, b, T.put(X, batched=True), T.put(Y, batched=True), idx, n_idx, M, 0.05, out_act, hidden)
        errs = [max(rel_err(dw.numpy(), w), rel_err(db.numpy(), bb)) for (w, bb), dw, db in zip(want, W, b)]
        lerr = rel_err(got_l, want_l)
        print("minibatch", sizes, hidden, out_act, dt.__name__, errs, "losses", lerr)
        assert max(errs) < RTOL[dt] and lerr < RTOL[dt]
        assert rel_err(W[0].numpy(), ws[0][0]) > 100 * RTOL[dt]     # the steps moved the parameters far beyond the tolerance


# ---- 7. contract ------------------------------------------------------------------------------------------------------------
def test_contract(Ts):
    from tensor_ops_amd import capi
    from tensor_ops_amd.hipt import Graph
    T = Ts[np.float32]
    L = capi.lib()
    N, M = 40, 8
    ws, X, Y = problem([30, 14, 6], N, np.float32, 0x77)
    W, b = put_net(T, ws)
    x, y = T.put(X, batched=True), T.put(Y, batched=True)
    poison = np.float32(-77.25)
    n_idx = 24
    losses = T.put(np.full(n_idx, poison, np.float32), batched=True)
    good = np.arange(n_idx, dtype=np.int64)

    def arr(ts):
        return (capi.c_tensor * len(ts))(*[t.h for t in ts])

    def status(Wl=W, bl=b, hidden="logistic", out_act="softmax", loss="crossEntropy", xx=x, yy=y, n=n_idx, idx=good, m=M,
               ll=losses):
        p = idx.ctypes.data_as(C.POINTER(C.c_int64)) if idx is not None else None
        st = L.to_fflayer_stack_minibatch_sgd(len(Wl), arr(Wl), arr(bl), HID[hidden], OUT[out_act], LOSS_ID[loss], xx.h,
                                              yy.h if yy is not None else None, n, p, m, 0.1, ll.h if ll is not None else None)
        assert st == OK or L.to_last_error() != b""
        return st

    def untouched(Wl=W, bl=b, wsl=ws):
        return (all(same_bits(dw.numpy(), w) and same_bits(db.numpy(), bb) for (w, bb), dw, db in zip(wsl, Wl, bl))
                and (losses.numpy() == poison).all())

    def with_idx(pos, v):
        i = good.copy()
        i[pos] = v
        return i

    refusals = [
        (dict(idx=with_idx(13, -1)), SHAPE),
        (dict(idx=with_idx(23, N)), SHAPE),
        (dict(m=0), ARG),
        (dict(n=0), ARG),
        (dict(yy=T.put(Y[:N - 1], batched=True)), SHAPE),
        (dict(ll=T.put(np.full(n_idx + 1, poison, np.float32), batched=True)), SHAPE),
        (dict(idx=None, n=N + 1, ll=None), SHAPE),
        (dict(loss="squaredError"), UNSUPPORTED),
        (dict(out_act="tanh"), UNSUPPORTED),
        (dict(out_act="tanh", loss="squaredError"), UNSUPPORTED),
    ]
    for kw, want in refusals:
        assert status(**kw) == want, kw
        assert untouched(), kw
    # a weight gradient outside the small-GEMM range (tests/test_gpu_stack_contract.py::test_refused_sgd_updates_nothing):
    # refused before the first of its three steps
    big = [832, 1024, 6]
    wsb, Xb, Yb = problem(big, N, np.float32, 0x78)
    Wb, bb = put_net(T, wsb)
    assert status(Wl=Wb, bl=bb, xx=T.put(Xb, batched=True), yy=T.put(Yb, batched=True)) == UNSUPPORTED
    assert untouched(Wb, bb, wsb)
    # the fp64 step's other refusal, "a contraction is outside the small-GEMM range" of its forward: [5, 70, 6] on 6337 rows
    # is 200 tiles of 64 x 64 in the hidden layer (tests/test_gpu_stack_tanh.py), the first count the fused kernel leaves
    T64 = Ts[np.float64]
    wsd, Xd, Yd = problem([5, 70, 6], 6337, np.float64, 0x79)
    Wd, bd = put_net(T64, wsd)
    xd, yd = T64.put(Xd, batched=True), T64.put(Yd, batched=True)
    twice = np.concatenate([np.arange(6337), np.arange(6337)]).astype(np.int64)
    assert status(Wl=Wd, bl=bd, xx=xd, yy=yd, idx=twice, n=len(twice), m=6337, ll=None) == UNSUPPORTED
    assert untouched(Wd, bd, wsd)
    # refused while a capture records; the capture goes on
    T.scaleT(3.0, x)
    with Graph() as g:
        st = status()
        h = T.scaleT(3.0, x)
    assert st == STATE and untouched()
    g.launch()
    assert np.array_equal(h.numpy(), 3 * X)
    # a good call: X and Y unchanged, no handle kept
    T.sync()
    live = T.stats()["live_handles"]
    assert status() == OK, L.to_last_error()
    T.sync()
    assert T.stats()["live_handles"] == live
    assert same_bits(x.numpy(), X) and same_bits(y.numpy(), Y)
    assert not untouched() and not (losses.numpy() == poison).any()
