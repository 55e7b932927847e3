"""Recurrent stacks over sequences of different lengths in one call (to_rnn_stack_run_ragged / _grad_ragged / _sgd_ragged,
csrc/rnn_ragged.hip): sequence b of X [B; T, i] is its first lens[b] steps, the rest is padding -- never read, written as
zero.

References: the masked fp64 numpy restatement (tests/rnn_ragged_numpy.py, itself checked in test_rnn_ragged_numpy_ref.py)
and the DENSE entries called per sequence on an upload of X[b, :lens[b]], gradients summed on the host.  Tolerances and
helpers are tests/test_gpu_rnn_stack.py's: TOL per dtype, k = 5 on what is summed over the batch."""
import ctypes as C

import numpy as np
import pytest

import rnn_ragged_numpy as RR
from test_gpu_rnn_stack import TOL, data, dev, make, put_seq, rel_err

pytestmark = pytest.mark.gpu
K = 5
LENS = [3, 1, 5, 5, 2, 4, 1]   # unsorted, ties, both extremes in one workgroup
T5 = 5
# (i, [(n, stateful)], out_act, loss): tests/test_gpu_rnn_stack.py's CASES, T raised to 5
P1 = (2, [(3, True)], "logistic", "squaredError")
P2 = (3, [(4, True), (5, False), (2, True)], "softmax", "crossEntropy")
P3 = (5, [(6, False), (7, True)], "softmax", "crossEntropy")
P4 = (9, [(37, True), (300, True), (11, False)], "softmax", "crossEntropy")
PARITY = [P1, P2, P3, P4]
DTYPES = [np.float32, np.float64]
case_id = lambda c: "i%d_L%d" % (c[0], len(c[1]))  # noqa: E731


@pytest.fixture(scope="module")
def Ts():
    from tensor_ops_amd.hipt import HipT
    return {np.float32: HipT(0, np.float32), np.float64: HipT(0, np.float64)}


@pytest.fixture(autouse=True)
def auto_route():
    from tensor_ops_amd.hipt import HipT
    prev = HipT.rnn_persistent(1)
    yield
    HipT.rnn_persistent(prev)


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def npz(ts):
    return [None if t is None else t.numpy() for t in ts]


def with_act(dl, sact):
    """device layers with a state activation on the stateful ones"""
    return [lay + (sact,) if lay[0] is not None and sact else lay for lay in dl]


def ragged(T, dl, x, y, lens, out_act, loss, hidden="logistic"):
    """every output of run_ragged and grad_ragged as numpy arrays"""
    out, fin = T.rnn_stack_run(dl, x, out_act, want_states=True, hidden_act=hidden, lens=lens)
    gS, gWS, gW, gB, gx, losses = T.rnn_stack_grad(dl, x, y, out_act, loss, want_gx=True, want_losses=True,
                                                   hidden_act=hidden, lens=lens)
    return {"out": out.numpy(), "s_out": npz(fin), "gs": npz(gS), "gws": npz(gWS), "gw": npz(gW), "gb": npz(gB),
            "gx": gx.numpy(), "losses": losses.numpy()}


def flat(r):
    """every array of a result, in a fixed order"""
    return [r["out"], r["gx"], r["losses"]] + [v for k in ("s_out", "gs", "gws", "gw", "gb") for v in r[k] if v is not None]


def dense_per_sequence(T, dl, X, Y, lens, out_act, loss, hidden="logistic"):
    """the dense entries on each sequence alone (B = 1 uploads of X[b, :lens[b]]); gradients summed in float64"""
    B, Tn = X.shape[:2]
    nL = Y.shape[2]
    n = len(dl)
    r = {"out": np.zeros((B, Tn, nL)), "gx": np.zeros(X.shape), "losses": np.zeros((B, Tn)),
         "s_out": [None if lay[0] is None else np.zeros((B, lay[2].shape[0])) for lay in dl]}
    for k in ("gs", "gws", "gw", "gb"):
        r[k] = [None] * n
    for q, ln in enumerate(lens):
        x, y = T.put(X[q, :ln]), T.put(Y[q, :ln])
        out, fin = T.rnn_stack_run(dl, x, out_act, want_states=True, hidden_act=hidden)
        g = T.rnn_stack_grad(dl, x, y, out_act, loss, want_gx=True, want_losses=True, hidden_act=hidden)
        r["out"][q, :ln] = out.numpy()
        r["gx"][q, :ln] = g[4].numpy()
        r["losses"][q, :ln] = g[5].numpy()
        for l in range(n):
            if fin[l] is not None:
                r["s_out"][l][q] = fin[l].numpy()
            for k, v in zip(("gs", "gws", "gw", "gb"), g[:4]):
                if v[l] is not None:
                    add = v[l].numpy().astype(np.float64)
                    r[k][l] = add if r[k][l] is None else r[k][l] + add
    return r


def numpy_reference(layers, X, Y, lens, out_act, loss):
    out, cache, _ = RR.forward(layers, X, lens, out_act)
    gs, gws, gw, gb, gx, losses = RR.bptt(layers, X, Y, lens, out_act, loss)
    return {"out": out, "s_out": RR.final_states(cache), "gs": gs, "gws": gws, "gw": gw, "gb": gb, "gx": gx, "losses": losses}


def check_against(got, want, tol, k, batched):
    shape = (lambda a: a) if batched else (lambda a: a[0])
    assert rel_err(got["out"], shape(want["out"])) < tol
    assert rel_err(got["gx"], shape(want["gx"])) < tol
    assert rel_err(got["losses"], shape(want["losses"])) < tol
    for l, w in enumerate(want["s_out"]):
        assert (w is None) == (got["s_out"][l] is None)
        if w is not None:
            assert rel_err(got["s_out"][l], shape(w)) < tol
    for name in ("gs", "gws", "gw", "gb"):
        for l, w in enumerate(want[name]):
            assert (w is None) == (got[name][l] is None), (name, l)
            if w is not None:
                assert rel_err(got[name][l], w) < k * tol, (name, l)


def padding_is_zero(r, lens, batched):
    m = RR.mask_of(lens, r["losses"].shape[-1])
    if not batched:
        m = m[0]
    for name in ("out", "gx", "losses"):
        pad = r[name][~m]
        assert bits_equal(pad, np.zeros_like(pad)), name   # +0.0, not -0.0


# ---- 1. parity ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("batched", [True, False], ids=["B7", "unbatched"])
@pytest.mark.parametrize("case", PARITY, ids=case_id)
def test_parity(Ts, dt, batched, case):
    T, tol = Ts[dt], TOL[dt]
    i, spec, out_act, loss = case
    lens = LENS if batched else [2]
    B = len(lens)
    k = K if batched else 1
    rng = np.random.default_rng(1000 + i + 17 * B)
    layers = make(rng, i, spec, dt)
    X, Y = data(rng, B, T5, i, spec[-1][0], dt)
    dl = dev(T, layers)
    x, y = put_seq(T, X, batched), put_seq(T, Y, batched)
    got = ragged(T, dl, x, y, lens, out_act, loss)
    padding_is_zero(got, lens, batched)
    want_np = numpy_reference(layers, X, Y, lens, out_act, loss)
    want_dense = dense_per_sequence(T, dl, X, Y, lens, out_act, loss)
    check_against(got, want_np, tol, k, batched)
    check_against(got, want_dense, tol, k, batched)
    # sgd: trainNetwork' on the masked objective, rate_state != rate_params
    rs, rp = 0.3, 0.05
    losses = T.rnn_stack_sgd(dl, x, y, rs, rp, out_act, loss, want_losses=True, lens=lens)
    assert rel_err(losses.numpy(), want_np["losses"] if batched else want_np["losses"][0]) < tol
    for want in (want_np, want_dense):
        for l, lay in enumerate(layers):
            for slot, name, rate in ((0, "gs", rs), (1, "gws", rp), (2, "gw", rp), (3, "gb", rp)):
                if lay[slot] is not None:
                    new = lay[slot].astype(np.float64) - rate * want[name][l]
                    assert rel_err(dl[l][slot].numpy(), new) < k * tol, (l, name)


# ---- 2. one tanh-state stack -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
def test_tanh_state_stack(Ts, dt):
    T, tol = Ts[dt], TOL[dt]
    rng = np.random.default_rng(21)
    layers = make(rng, 6, [(8, True), (4, False)], dt)
    X, Y = data(rng, 7, T5, 6, 4, dt)
    dl = with_act(dev(T, layers), "tanh")
    got = ragged(T, dl, T.put(X, batched=True), T.put(Y, batched=True), LENS, "softmax", "crossEntropy", hidden="tanh")
    padding_is_zero(got, LENS, True)
    check_against(got, dense_per_sequence(T, dl, X, Y, LENS, "softmax", "crossEntropy", hidden="tanh"), tol, K, True)


# ---- 3. both routes ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
def test_both_routes(Ts, dt):
    from tensor_ops_amd.hipt import HipT
    T, tol = Ts[dt], TOL[dt]
    i, spec, out_act, loss = P4
    rng = np.random.default_rng(31)
    layers = make(rng, i, spec, dt)
    X, Y = data(rng, 7, T5, i, spec[-1][0], dt)
    dl = dev(T, layers)
    x, y = T.put(X, batched=True), T.put(Y, batched=True)
    want = numpy_reference(layers, X, Y, LENS, out_act, loss)
    got = {}
    for mode in (0, 2):
        HipT.rnn_persistent(mode)
        r0, d0 = HipT.rnn_ragged_stats(), HipT.rnn_stats()
        got[mode] = ragged(T, dl, x, y, LENS, out_act, loss)
        r1, d1 = HipT.rnn_ragged_stats(), HipT.rnn_stats()
        assert (r1[0] - r0[0], r1[1] - r0[1]) == ((2, 0) if mode == 2 else (0, 2))
        assert d1 == d0   # the dense counters do not move
        check_against(got[mode], want, tol, K, True)
    for name, k in (("out", 1), ("gx", 1), ("losses", 1)):
        assert rel_err(got[0][name], got[2][name]) < k * tol
    for name in ("gs", "gws", "gw", "gb"):
        for a, b in zip(got[0][name], got[2][name]):
            if a is not None:
                assert rel_err(a, b) < K * tol
    # automatic: H = 37 fits the kernel's LDS, H = 300 does not -- the call counts as per step
    HipT.rnn_persistent(1)
    r0 = HipT.rnn_ragged_stats()
    T.rnn_stack_run(dl, x, out_act, lens=LENS)
    r1 = HipT.rnn_ragged_stats()
    assert (r1[0] - r0[0], r1[1] - r0[1]) == (0, 1)


# ---- 4. padding is never read, and is written as zero ---------------------------------------------------------------------
def sentinel_run(T, dl, X, Y, lens, out_act, loss, dt):
    """run_ragged and grad_ragged through the C ABI into destinations pre-filled with 7.0"""
    from tensor_ops_amd import capi
    from tensor_ops_amd.hipt import HipT
    L = capi.lib()
    B, Tn, i = X.shape
    nL = Y.shape[2]
    x, y = T.put(X, batched=True), T.put(Y, batched=True)
    seven = lambda shape, batched=False: T.put(np.full(shape, 7.0, dt), batched=batched)  # noqa: E731
    out = seven((B, Tn, nL), True)
    gx = seven((B, Tn, i), True)
    losses = seven((B, Tn), True)
    fin = [None if lay[0] is None else seven((B, lay[2].shape[0]), True) for lay in dl]
    gS = [None if lay[0] is None else seven(lay[0].shape) for lay in dl]
    gWS = [None if lay[1] is None else seven(lay[1].shape) for lay in dl]
    gW = [seven(lay[2].shape) for lay in dl]
    gB = [seven(lay[3].shape) for lay in dl]
    n, sact, (s, ws, w, b) = HipT._rnn_arrays(dl)
    arr = lambda ts: (capi.c_tensor * n)(*[(t.h if t is not None else None) for t in ts])  # noqa: E731
    la = np.asarray(lens, np.int64)
    lp = la.ctypes.data_as(C.POINTER(C.c_int64))
    oa, ls = HipT._RNN_OUT[out_act], HipT._RNN_LOSS[loss]
    assert L.to_rnn_stack_run_ragged(n, sact, s, ws, w, b, 0, oa, x.h, lp, out.h, arr(fin)) == 0
    assert L.to_rnn_stack_grad_ragged(n, sact, s, ws, w, b, 0, oa, ls, x.h, y.h, lp, arr(gS), arr(gWS), arr(gW), arr(gB),
                                      gx.h, losses.h) == 0
    return {"out": out.numpy(), "s_out": npz(fin), "gs": npz(gS), "gws": npz(gWS), "gw": npz(gW), "gb": npz(gB),
            "gx": gx.numpy(), "losses": losses.numpy()}


@pytest.mark.parametrize("mode", [2, 0], ids=["persistent", "per_step"])
@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
def test_padding_is_never_read_and_written_as_zero(Ts, dt, mode):
    from tensor_ops_amd.hipt import HipT
    T = Ts[dt]
    i, spec, out_act, loss = P2
    rng = np.random.default_rng(41)
    layers = make(rng, i, spec, dt)
    X, Y = data(rng, 7, T5, i, spec[-1][0], dt)
    m = RR.mask_of(LENS, T5)
    X0, Y0, Xn, Yn = X.copy(), Y.copy(), X.copy(), Y.copy()
    X0[~m], Y0[~m], Xn[~m], Yn[~m] = 0.0, 0.0, np.nan, np.nan
    dl = dev(T, layers)
    HipT.rnn_persistent(mode)
    zero = sentinel_run(T, dl, X0, Y0, LENS, out_act, loss, dt)
    nan = sentinel_run(T, dl, Xn, Yn, LENS, out_act, loss, dt)
    for a, b in zip(flat(zero), flat(nan)):
        assert bits_equal(a, b) and np.isfinite(b).all()
    padding_is_zero(nan, LENS, True)
    check_against(nan, numpy_reference(layers, Xn, Yn, LENS, out_act, loss), TOL[dt], K, True)   # (and no sentinel is left)


# ---- 5. all lengths equal to T: the dense entry, bit for bit --------------------------------------------------------------
@pytest.mark.parametrize("mode", [2, 0], ids=["persistent", "per_step"])
@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("case", [P2, P4], ids=case_id)
def test_all_lengths_T_is_the_dense_entry_bit_for_bit(Ts, dt, mode, case):
    from tensor_ops_amd.hipt import HipT
    T = Ts[dt]
    i, spec, out_act, loss = case
    B, Tn = 7, 4
    rng = np.random.default_rng(51)
    layers = make(rng, i, spec, dt)
    X, Y = data(rng, B, Tn, i, spec[-1][0], dt)
    dl = dev(T, layers)
    x, y = T.put(X, batched=True), T.put(Y, batched=True)
    HipT.rnn_persistent(mode)
    got = ragged(T, dl, x, y, [Tn] * B, out_act, loss)
    out, fin = T.rnn_stack_run(dl, x, out_act, want_states=True)
    gS, gWS, gW, gB, gx, losses = T.rnn_stack_grad(dl, x, y, out_act, loss, want_gx=True, want_losses=True)
    dense = {"out": out.numpy(), "s_out": npz(fin), "gs": npz(gS), "gws": npz(gWS), "gw": npz(gW), "gb": npz(gB),
             "gx": gx.numpy(), "losses": losses.numpy()}
    for a, b in zip(flat(got), flat(dense)):
        assert bits_equal(a, b)


# ---- 6. order ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [2, 0], ids=["persistent", "per_step"])
def test_order_of_the_sequences(Ts, mode):
    from tensor_ops_amd.hipt import HipT
    dt = np.float32
    T, tol = Ts[dt], TOL[dt]
    i, spec, out_act, loss = P4
    rng = np.random.default_rng(61)
    layers = make(rng, i, spec, dt)
    X, Y = data(rng, 7, T5, i, spec[-1][0], dt)
    dl = dev(T, layers)
    HipT.rnn_persistent(mode)
    lens = np.asarray(LENS)
    a = ragged(T, dl, T.put(X, batched=True), T.put(Y, batched=True), lens, out_act, loss)
    again = ragged(T, dl, T.put(X, batched=True), T.put(Y, batched=True), lens, out_act, loss)
    for u, v in zip(flat(a), flat(again)):
        assert bits_equal(u, v)
    perm = np.array([4, 2, 6, 0, 5, 1, 3])
    b = ragged(T, dl, T.put(X[perm], batched=True), T.put(Y[perm], batched=True), lens[perm], out_act, loss)
    for name in ("out", "gx", "losses"):
        assert rel_err(b[name], a[name][perm]) < tol
    for u, v in zip(a["s_out"], b["s_out"]):
        if u is not None:
            assert rel_err(v, u[perm]) < tol
    for name in ("gs", "gws", "gw", "gb"):
        for u, v in zip(a[name], b[name]):
            if u is not None:
                assert rel_err(v, u) < K * tol


# ---- 7. launch counts ------------------------------------------------------------------------------------------------------
def test_launch_counts(Ts):
    from tensor_ops_amd.hipt import HipT
    dt = np.float32
    T = Ts[dt]
    rng = np.random.default_rng(71)
    layers = make(rng, 6, [(8, True), (4, False)], dt)
    dl = dev(T, layers)

    def launches(Tn, lens):
        X, Y = data(rng, 7, Tn, 6, 4, dt)
        x, y = T.put(X, batched=True), T.put(Y, batched=True)
        T.rnn_stack_grad(dl, x, y, want_gx=True, lens=lens)
        l0 = T.stats()["launches"]
        T.rnn_stack_grad(dl, x, y, want_gx=True, lens=lens)
        return T.stats()["launches"] - l0
    short = [3, 1, 4, 4, 2, 4, 1]
    HipT.rnn_persistent(2)   # persistent: independent of T and of the lengths
    a, b = launches(4, short), launches(32, [17, 1, 32, 9, 32, 4, 25])
    assert a == b, (a, b)
    HipT.rnn_persistent(0)   # per step: max(lens) counts, T does not
    a, b = launches(4, short), launches(32, short)
    assert a == b, (a, b)
    assert launches(32, [3, 1, 8, 4, 2, 4, 1]) > b


# ---- 8. chunked run ------------------------------------------------------------------------------------------------------
def test_chunked_run(Ts):
    dt = np.float32
    T, tol = Ts[dt], TOL[dt]
    rng = np.random.default_rng(81)
    layers = make(rng, 5, [(24, True), (6, False), (9, True)], dt)
    dl = dev(T, layers)
    lens = np.array([5, 2, 4])
    X, _ = data(rng, 3, T5, 5, 9, dt)
    whole, fin = T.rnn_stack_run(dl, T.put(X, batched=True), "logistic", want_states=True, lens=lens)
    a, fa = T.rnn_stack_run(dl, T.put(X[:, :2], batched=True), "logistic", want_states=True, lens=np.minimum(lens, 2))
    go_on = [0, 2]   # the sequences with steps left: lens - 2 = [3, 2], a batch of their own, from their own states
    dl2 = [(T.put(fa[l].numpy()[go_on], batched=True), lay[1], lay[2], lay[3]) if lay[0] is not None else lay
           for l, lay in enumerate(dl)]
    b, fb = T.rnn_stack_run(dl2, T.put(X[go_on, 2:], batched=True), "logistic", want_states=True, lens=lens[go_on] - 2)
    whole = whole.numpy()
    assert rel_err(a.numpy(), whole[:, :2]) < tol
    assert rel_err(b.numpy(), whole[go_on, 2:]) < tol
    for l in (0, 2):
        assert rel_err(fb[l].numpy(), fin[l].numpy()[go_on]) < tol
        assert rel_err(fa[l].numpy()[1], fin[l].numpy()[1]) < tol   # the sequence that ended in the first chunk


# ---- 9. contract ---------------------------------------------------------------------------------------------------------
def test_contract(Ts):
    from tensor_ops_amd import capi
    from tensor_ops_amd.hipt import Graph
    L = capi.lib()
    T, T64 = Ts[np.float32], Ts[np.float64]
    rng = np.random.default_rng(91)
    layers = make(rng, 4, [(6, True), (3, False)], np.float32)
    dl = dev(T, layers)
    B, Tn = 5, 4
    X, Y = data(rng, B, Tn, 4, 3, np.float32)
    x, y = T.put(X, batched=True), T.put(Y, batched=True)
    good = [2, 4, 1, 3, 4]
    n = len(dl)
    arr = lambda k: (capi.c_tensor * n)(*[(lay[k].h if lay[k] is not None else None) for lay in dl])  # noqa: E731
    sact = (C.c_int * n)(0, -1)
    before = [[None if v is None else v.numpy() for v in lay] for lay in dl]

    def lp(lens):
        if lens is None:
            return None, None
        a = np.asarray(lens, np.int64)
        return a, a.ctypes.data_as(C.POINTER(C.c_int64))

    def seven(shape, TT=T, dt=np.float32):
        return TT.put(np.full(shape, 7.0, dt), batched=True)

    def untouched(*ts):
        for t in ts:
            v = t.numpy()
            assert bits_equal(v, np.full(v.shape, 7.0, v.dtype))
        for lay, want in zip(dl, before):
            for v, w in zip(lay, want):
                if v is not None:
                    assert bits_equal(v.numpy(), w)

    # each helper allocates its sentinel-filled destinations and returns (the call, the destinations)
    def run(lens=good, out=None, out_act=2):
        out = seven((B, Tn, 3)) if out is None else out
        fin = seven((B, 6))
        keep, p = lp(lens)
        s_out = (capi.c_tensor * n)(fin.h, None)
        return (lambda: (keep, L.to_rnn_stack_run_ragged(n, sact, arr(0), arr(1), arr(2), arr(3), 0, out_act, x.h, p, out.h,
                                                          s_out))[1]), [out, fin]

    def grad(lens=good, out_act=2, loss=1):
        gS, gWS = [T.put(np.full(6, 7.0, np.float32)), None], [T.put(np.full((6, 6), 7.0, np.float32)), None]
        gW = [T.put(np.full(lay[2].shape, 7.0, np.float32)) for lay in dl]
        gB = [T.put(np.full(lay[3].shape, 7.0, np.float32)) for lay in dl]
        gx, losses = seven((B, Tn, 4)), seven((B, Tn))
        keep, p = lp(lens)
        h = lambda ts: (capi.c_tensor * n)(*[(t.h if t is not None else None) for t in ts])  # noqa: E731
        return (lambda: (keep, L.to_rnn_stack_grad_ragged(n, sact, arr(0), arr(1), arr(2), arr(3), 0, out_act, loss, x.h, y.h,
                                                           p, h(gS), h(gWS), h(gW), h(gB), gx.h, losses.h))[1]), \
            [t for t in gS + gWS + gW + gB if t is not None] + [gx, losses]

    def sgd(lens=good, out_act=2, loss=1):
        losses = seven((B, Tn))
        keep, p = lp(lens)
        return (lambda: (keep, L.to_rnn_stack_sgd_ragged(n, sact, arr(0), arr(1), arr(2), arr(3), 0, out_act, loss, x.h, y.h, p,
                                                          0.1, 0.1, losses.h))[1]), [losses]

    def refused(made, status, dests=None):
        call, own = made
        assert call() == status
        untouched(*(own if dests is None else dests))

    for lens, status in ((None, 1), ([2, 4, 0, 3, 4], 2), ([2, 4, 1, Tn + 1, 4], 2)):   # null: ARG; 0 or T + 1: SHAPE
        for make_call in (run, grad, sgd):
            refused(make_call(lens=lens), status)
    refused(run(out=seven((B, Tn, 3), T64, np.float64)), 1)              # dtype mismatch: the dense status
    base = seven((B, 3, Tn))                                             # a transposed view: [B; Tn, 3], not contiguous
    made = run(out=T.transp(base))
    refused(made, 1, [base, made[1][1]])                                 # the dense status
    for make_call in (grad, sgd):
        for pair in ((2, 0), (0, 1)):                                    # (out_act, loss) outside the contract
            refused(make_call(out_act=pair[0], loss=pair[1]), 5)
    made = [run(), grad(), sgd()]
    with Graph():
        st = [m[0]() for m in made]
    assert st == [4, 4, 4]                                               # refused while a capture records
    untouched(*[t for m in made for t in m[1]])
    # and the calls work: T = 1 with lens = [1] * B
    x1 = T.put(X[:, :1], batched=True)
    out1, _ = T.rnn_stack_run(dl, x1, "softmax", lens=[1] * B)
    dense1, _ = T.rnn_stack_run(dl, x1, "softmax")
    assert bits_equal(out1.numpy(), dense1.numpy())
    assert sgd()[0]() == 0
    assert not np.array_equal(dl[0][1].numpy(), before[0][1])

