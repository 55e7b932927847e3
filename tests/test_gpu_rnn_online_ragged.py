"""Per-sequence training of sequences of different lengths in one call (to_rnn_stack_online_sgd_ragged, csrc/rnn_online.hip):
`trainNetwork'` folded over the sequences idx[0 .. n_idx) of a resident, padded set, step j on the leading lens[idx[j]] steps
of its sequence alone, on both routes (to_set_rnn_online_persistent 0: per sequence, 2: the persistent kernel, 1: automatic).

Checked against the float64 restatement tests/rnn_online_ragged_numpy.py (held to oracle/recurrent.py's trainNetwork at 1e-10
by tests/test_rnn_online_ragged_numpy_ref.py).  Tolerance: tests/test_gpu_rnn_tanh.py's TOL (1e-5 / 1e-11 relative l2) times
its factor 5, the dense online test's bound for chains of at most 5 updates.  The chains do not amplify: on the CPU, for
exactly these cases, the restatement with the parameters rounded to fp32 after every update stays within 8e-8 of the
unrounded one, the parameters stay below 1.8 in magnitude and everything is finite.  The cases put a short sequence straight
behind a long one (5, 2, 1 steps in "mixed"; 600 then 37; 40 then 9), a sequence of one step (no backward recurrence at all)
among them: what the longer one left on the kernel's tape must be read by nothing.  Then: NaN in every padding row changes
no bit, equal lengths give the dense entry's bits, route A is the caller's own loop bit for bit, cutting a chain into two
calls and repeating a call give identical bits on both routes, the launch count of the persistent route depends neither on
n_idx nor on T nor on the lengths, a stack beyond the kernel's LDS runs per sequence, the contract, and a NaN inside a
sequence.

Measured on an MI355X (max over parameters, states and losses of the relative l2 error against the restatement, max over
the cases and hidden activations; printed by test_parity): route A 1.6e-7 in fp32 and 4.8e-16 in fp64, route B 1.8e-7 and 1.5e-16; the bounds are 5e-5 and
5e-11."""
import ctypes as C
import functools

import numpy as np
import pytest

import rnn_online_ragged_numpy as ORN
from test_gpu_rnn_tanh import LOSS, TOL, dev, make, rel_err

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
H_STAR = 128   # include/tensorops_hip.h: automatic = route B where the plan fits and no layer is wider

WIDE = (70, [(130, "logistic"), (3, None)], "softmax")
# name: (i, [(n, state_act)], out_act, T, N, idx, lens, dtypes, (rate_state, rate_params), dtypes whose plan fits the kernel's LDS)
CASES = {
    # full length, one step, and long -> short -> shorter (5, 2, 1 steps) in a row
    "mixed": (7, [(12, "tanh"), (9, "logistic"), (5, None)], "softmax", 5, 6, [3, 0, 3, 5, 1], [5, 1, 3, 2, 4, 1], [F32, F64],
              (0.3, 0.05), [F32, F64]),
    # a stateful output layer under the logistic head, and an immediate repeat
    "state_head": (6, [(6, "tanh")], "logistic", 4, 4, [1, 1, 3, 0], [4, 2, 3, 1], [F32, F64], (0.3, 0.05), [F32, F64]),
    # widths above 64 and 128 that are no multiples of 64; in fp64 the parameters exceed the LDS: no plan
    "wide": WIDE + (3, 3, [0, 2, 1], [1, 3, 2], [F32, F64], (0.3, 0.05), [F32]),
    # 37 steps, then 600, then 37 again over the 600 records the long one left; the tape in LDS
    "longT": (3, [(4, "tanh"), (3, None)], "softmax", 600, 2, [1, 0, 1], [600, 37], [F32, F64], (0.01, 0.002), [F32, F64]),
    # the longest sequence used has 40 steps: 40 records of 472 elements do not fit beside the parameters, the tape is in
    # global memory
    "wide_T40": WIDE + (40, 2, [1, 0, 1], [40, 9], [F32], (0.01, 0.002), [F32]),
    # the same set, but only the sequence of 9 steps is trained on: the plan follows the longest length USED, the tape is in LDS
    "wide_short": WIDE + (40, 2, [1, 1], [40, 9], [F32], (0.01, 0.002), [F32]),
}


@pytest.fixture(scope="module")
def Ts():
    from tensor_ops_amd.hipt import HipT
    return {F32: HipT(0, F32), F64: HipT(0, F64)}


@pytest.fixture(autouse=True)
def auto_route():
    from tensor_ops_amd.hipt import HipT
    prev = HipT.rnn_online_persistent(1)
    yield
    HipT.rnn_online_persistent(prev)


@functools.lru_cache(maxsize=None)
def data(name, dt):
    i, spec, out_act, T, N = CASES[name][:5]
    rng = np.random.default_rng(0x61 + T + N + len(name))
    layers = make(rng, i, spec, dt)
    X = rng.uniform(-1, 1, (N, T, i)).astype(dt)
    Y = rng.uniform(0.1, 0.9, (N, T, spec[-1][0])).astype(dt)
    return layers, X, Y


@functools.lru_cache(maxsize=None)
def reference(name, dt, hidden):
    """computed once per (case, dtype, hidden activation) and shared; nobody writes to it"""
    layers, X, Y = data(name, dt)
    out_act, idx, lens, rates = CASES[name][2], CASES[name][5], CASES[name][6], CASES[name][8]
    return ORN.online(layers, X, Y, lens, idx, rates[0], rates[1], hidden, out_act)


def expect_persistent(name, dt, mode):
    spec, fits = CASES[name][1], dt in CASES[name][9]
    return fits and (mode == 2 or (mode == 1 and max(n for n, _ in spec) <= H_STAR))


def errors(dl, losses, want_layers, want_losses):
    errs = []
    for l, want in enumerate(want_layers):
        errs += [rel_err(dl[l][2].numpy(), want[2]), rel_err(dl[l][3].numpy(), want[3])]
        if want[1] is not None:
            errs += [rel_err(dl[l][0].numpy(), want[0]), rel_err(dl[l][1].numpy(), want[1])]
        else:
            assert dl[l][0] is None and dl[l][1] is None   # a stateless layer keeps its null state entries
    return errs + [rel_err(losses.numpy(), want_losses)]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def all_bits(dl, losses):
    out = [bits(t.numpy()) for lay in dl for t in lay[:4] if t is not None]
    return out + ([bits(losses.numpy())] if losses is not None else [])


def same(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b))


def poisoned(X, Y, lens):
    """NaN in every padding row"""
    Xn, Yn = X.copy(), Y.copy()
    for q, n in enumerate(lens):
        Xn[q, n:] = np.nan
        Yn[q, n:] = np.nan
    return Xn, Yn


PARITY = [(name, dt, hidden, mode) for name, c in CASES.items() for dt in c[7] for hidden in ("tanh", "logistic")
          for mode in (0, 1, 2)]


def ident(v):
    return getattr(v, "__name__", str(v))


@pytest.mark.parametrize("name,dt,hidden,mode", PARITY, ids=ident)
def test_parity(Ts, name, dt, hidden, mode):
    from tensor_ops_amd.hipt import HipT
    i, spec, out_act, n, N, idx, lens, _, (rs, rp), _ = CASES[name]
    T = Ts[dt]
    layers, X, Y = data(name, dt)
    want_layers, want_losses = reference(name, dt, hidden)
    HipT.rnn_online_persistent(mode)
    dl = dev(T, layers)
    p0, d0 = HipT.rnn_online_ragged_stats(), HipT.rnn_online_stats()
    losses = T.rnn_stack_online_sgd_ragged(dl, T.put(X, batched=True), T.put(Y, batched=True), lens, rs, rp, idx=idx,
                                           out_act=out_act, loss=LOSS[out_act], hidden_act=hidden, want_losses=True)
    p1 = HipT.rnn_online_ragged_stats()
    assert (p1[0] - p0[0], p1[1] - p0[1]) == ((1, 0) if expect_persistent(name, dt, mode) else (0, 1))
    assert HipT.rnn_online_stats() == d0   # the dense entry's counters did not move
    ls = losses.numpy()
    assert ls.shape == (len(idx), n)
    for j, q in enumerate(idx):   # +0.0 at the padding, bit for bit
        assert not bits(ls[j, lens[q]:]).any(), (j, q)
    errs = errors(dl, losses, want_layers, want_losses)
    print(name, ident(dt), hidden, "mode", mode, "max error", max(errs))
    assert max(errs) < 5 * TOL[dt]


@pytest.mark.parametrize("dt", [F32, F64], ids=ident)
@pytest.mark.parametrize("mode", [0, 2], ids=["per_sequence", "persistent"])
def test_padding_is_never_read(Ts, dt, mode):
    """NaN in every padding row of X and Y: every bit of every parameter, state and loss is the clean run's"""
    from tensor_ops_amd.hipt import HipT
    i, spec, out_act, n, N, idx, lens, _, (rs, rp), _ = CASES["mixed"]
    T = Ts[dt]
    layers, X, Y = data("mixed", dt)
    Xn, Yn = poisoned(X, Y, lens)
    assert np.isnan(Xn).any() and np.isnan(Yn).any()
    HipT.rnn_online_persistent(mode)

    def run(xx, yy):
        dl = dev(T, layers)
        losses = T.rnn_stack_online_sgd_ragged(dl, T.put(xx, batched=True), T.put(yy, batched=True), lens, rs, rp, idx=idx,
                                               out_act=out_act, loss=LOSS[out_act], hidden_act="tanh", want_losses=True)
        return all_bits(dl, losses)
    clean = run(X, Y)
    assert same(run(Xn, Yn), clean)
    assert not any(np.isnan(a.view(dt)).any() for a in clean)


@pytest.mark.parametrize("dt", [F32, F64], ids=ident)
@pytest.mark.parametrize("mode", [0, 2], ids=["per_sequence", "persistent"])
@pytest.mark.parametrize("name", ["mixed", "state_head"])
def test_equal_lengths_are_the_dense_entry(Ts, name, dt, mode):
    from tensor_ops_amd.hipt import HipT
    i, spec, out_act, n, N, idx, _, _, (rs, rp), _ = CASES[name]
    T = Ts[dt]
    layers, X, Y = data(name, dt)
    x, y = T.put(X, batched=True), T.put(Y, batched=True)
    HipT.rnn_online_persistent(mode)
    kw = dict(idx=idx, out_act=out_act, loss=LOSS[out_act], hidden_act="tanh", want_losses=True)
    a, b = dev(T, layers), dev(T, layers)
    la = T.rnn_stack_online_sgd_ragged(a, x, y, [n] * N, rs, rp, **kw)
    lb = T.rnn_stack_online_sgd(b, x, y, rs, rp, **kw)
    assert same(all_bits(a, la), all_bits(b, lb))


def wrapped_rows(T, t, q, rows):
    """the leading `rows` rows of sequence q of the batched [N; T, n] t, as a to_wrap view at t's own device address"""
    from tensor_ops_amd import capi
    from tensor_ops_amd.hipt import DT
    (n_t, n), es = t.shape, np.dtype(T.dtype).itemsize
    dims, rank = capi.dims_arr((rows, n))
    h = capi.c_tensor()
    capi.check(capi.lib().to_wrap(C.c_void_p(t.ptr + q * n_t * n * es), T.to_dtype, rank, dims, 0, C.byref(h)))
    return DT(h)


@pytest.mark.parametrize("dt", [F32, F64], ids=ident)
@pytest.mark.parametrize("name", ["mixed", "state_head"])
def test_route_a_is_the_callers_loop(Ts, name, dt):
    """mode 0: bit for bit a Python loop of rnn_stack_sgd over to_wrap views of the leading rows at X's and Y's own addresses"""
    from tensor_ops_amd.hipt import HipT
    i, spec, out_act, n, N, idx, lens, _, (rs, rp), _ = CASES[name]
    T = Ts[dt]
    layers, X, Y = data(name, dt)
    x, y = T.put(X, batched=True), T.put(Y, batched=True)
    HipT.rnn_online_persistent(0)
    for hidden in ("tanh", "logistic"):
        dl = dev(T, layers)
        losses = T.rnn_stack_online_sgd_ragged(dl, x, y, lens, rs, rp, idx=idx, out_act=out_act, loss=LOSS[out_act],
                                               hidden_act=hidden, want_losses=True)
        dl2, rows = dev(T, layers), np.zeros((len(idx), n), dt)
        for j, q in enumerate(idx):
            ls = T.rnn_stack_sgd(dl2, wrapped_rows(T, x, q, lens[q]), wrapped_rows(T, y, q, lens[q]), rs, rp, out_act,
                                 LOSS[out_act], want_losses=True, hidden_act=hidden)
            rows[j, :lens[q]] = ls.numpy()
        assert same(all_bits(dl, None), all_bits(dl2, None))
        assert np.array_equal(bits(losses.numpy()), bits(rows))


@pytest.mark.parametrize("dt", [F32, F64], ids=ident)
@pytest.mark.parametrize("mode", [0, 2], ids=["per_sequence", "persistent"])
def test_cutting_and_determinism(Ts, dt, mode):
    from tensor_ops_amd.hipt import HipT
    i, spec, out_act, n, N, idx, lens, _, (rs, rp), _ = CASES["mixed"]
    T = Ts[dt]
    layers, X, Y = data("mixed", dt)
    x, y = T.put(X, batched=True), T.put(Y, batched=True)
    HipT.rnn_online_persistent(mode)

    def run(dl, ii, n_idx=None):
        return T.rnn_stack_online_sgd_ragged(dl, x, y, lens, rs, rp, idx=ii, n_idx=n_idx, out_act=out_act, loss=LOSS[out_act],
                                             hidden_act="tanh", want_losses=True)
    whole = dev(T, layers)
    lw = run(whole, idx)
    # two identical calls from identical starts
    again = dev(T, layers)
    la = run(again, idx)
    assert same(all_bits(whole, lw), all_bits(again, la))
    # n_idx = 2, then the remaining 3 from the first call's parameters
    cut = dev(T, layers)
    l1 = run(cut, idx[:2])
    l2 = run(cut, idx[2:])
    assert same(all_bits(whole, None), all_bits(cut, None))
    assert np.array_equal(bits(lw.numpy()), bits(np.concatenate([l1.numpy(), l2.numpy()])))
    # idx null is idx = arange
    a, b = dev(T, layers), dev(T, layers)
    l_null = run(a, None, n_idx=4)
    l_arange = run(b, np.arange(4))
    assert same(all_bits(a, l_null), all_bits(b, l_arange))
    assert not same(all_bits(a, None), all_bits(dev(T, layers), None))   # (something was trained)


@pytest.mark.parametrize("dt", [F32, F64], ids=ident)
def test_one_launch(Ts, dt):
    from tensor_ops_amd.hipt import HipT
    i, spec, out_act = CASES["mixed"][:3]
    T = Ts[dt]
    rng = np.random.default_rng(5)
    layers = make(rng, i, spec, dt)

    def launches(n_idx, n, lens):
        X = rng.uniform(-1, 1, (6, n, i)).astype(dt)
        Y = rng.uniform(0.1, 0.9, (6, n, spec[-1][0])).astype(dt)
        x, y, dl = T.put(X, batched=True), T.put(Y, batched=True), dev(T, layers)
        idx = np.arange(n_idx) % 6
        T.rnn_stack_online_sgd_ragged(dl, x, y, lens, 0.3, 0.05, idx=idx, out_act=out_act)
        l0 = T.stats()["launches"]
        T.rnn_stack_online_sgd_ragged(dl, x, y, lens, 0.3, 0.05, idx=idx, out_act=out_act)
        return T.stats()["launches"] - l0
    short, other = [1, 2, 1, 3, 2, 1], [9, 4, 1, 7, 2, 5]
    HipT.rnn_online_persistent(2)
    a, b = launches(2, 3, short), launches(7, 9, other)
    assert a == b, (a, b)
    HipT.rnn_online_persistent(0)
    assert launches(2, 3, short) < launches(7, 3, short)   # the per-sequence route grows with n_idx


def test_out_of_range(Ts):
    """fp32 64 -> 160 (tanh) -> 64: 182 KiB of parameters, no plan: per sequence even when route B is forced -- and right"""
    from tensor_ops_amd.hipt import HipT
    T, dt = Ts[F32], F32
    rng = np.random.default_rng(0x33)
    layers = make(rng, 64, [(160, "tanh"), (64, None)], dt)
    X = rng.uniform(-1, 1, (2, 2, 64)).astype(dt)
    Y = rng.uniform(0.1, 0.9, (2, 2, 64)).astype(dt)
    idx, lens = [1, 0], [2, 1]
    want_layers, want_losses = ORN.online(layers, X, Y, lens, idx, 0.3, 0.05, "logistic", "softmax")
    HipT.rnn_online_persistent(2)
    dl = dev(T, layers)
    p0 = HipT.rnn_online_ragged_stats()
    losses = T.rnn_stack_online_sgd_ragged(dl, T.put(X, batched=True), T.put(Y, batched=True), lens, 0.3, 0.05, idx=idx,
                                           want_losses=True)
    p1 = HipT.rnn_online_ragged_stats()
    assert (p1[0] - p0[0], p1[1] - p0[1]) == (0, 1)
    errs = errors(dl, losses, want_layers, want_losses)
    print("out of range: max error", max(errs))
    assert max(errs) < 5 * TOL[dt]


def test_contract(Ts):
    from tensor_ops_amd import capi
    from tensor_ops_amd.hipt import Graph, HipT
    L = capi.lib()
    T, dt = Ts[F32], F32
    i, spec, out_act, n, N, idx, lens, _, (rs, rp), _ = CASES["mixed"]
    layers, X, Y = data("mixed", dt)
    dl = dev(T, layers)
    x, y = T.put(X, batched=True), T.put(Y, batched=True)
    n_idx = len(idx)
    sentinel = lambda *shape: T.put(np.full(shape, 7.5, dt), batched=True)  # noqa: E731
    losses = sentinel(n_idx, n)
    start = all_bits(dl, losses)
    ARG, SHAPE, STATE, UNSUPPORTED = 1, 2, 4, 5
    i64 = lambda v: np.ascontiguousarray(v, np.int64).ctypes.data_as(C.POINTER(C.c_int64))  # noqa: E731

    def call(layers_=dl, xx=x, yy=y, k=n_idx, ii=idx, out_act_=2, loss_=1, ll=losses, sact=(3, 0, -1), nn=lens):
        nl = len(layers_)
        arr = lambda c: (capi.c_tensor * nl)(*[(lay[c].h if lay[c] is not None else None) for lay in layers_])  # noqa
        ia = np.ascontiguousarray(ii, np.int64) if ii is not None else None
        na = np.ascontiguousarray(nn, np.int64) if nn is not None else None
        return L.to_rnn_stack_online_sgd_ragged(nl, (C.c_int * nl)(*sact), arr(0), arr(1), arr(2), arr(3), 0, out_act_, loss_,
                                                xx.h, yy.h, i64(na) if na is not None else None, k,
                                                i64(ia) if ia is not None else None, rs, rp,
                                                ll if isinstance(ll, (int, type(None))) else ll.h)
    HipT.rnn_online_persistent(2)   # route B's validation is the one exercised
    assert call(k=0, ii=None) == ARG                                             # n_idx = 0
    assert call(ii=[3, 0, N, 5, 1]) == SHAPE and call(ii=[3, 0, -1, 5, 1]) == SHAPE   # an index out of range
    assert call(k=N + 1, ii=None, ll=sentinel(N + 1, n)) == SHAPE                # idx null with n_idx > N
    assert call(xx=T.put(X[0])) == SHAPE                                         # unbatched X
    assert call(yy=T.put(Y[:, :n - 1], batched=True)) == SHAPE                   # Y of another T
    assert call(ll=sentinel(n_idx + 1, n)) == SHAPE                              # losses of the wrong batch
    batched_s = [(T.put(np.tile(layers[0][0], (N, 1)), batched=True),) + dl[0][1:]] + dl[1:]
    assert call(layers_=batched_s) == SHAPE                                      # a batched initial state
    assert call(out_act_=3) == UNSUPPORTED                                       # tanh as out_act
    assert call(loss_=0) == UNSUPPORTED                                          # a softmax / squaredError pair
    alias = capi.c_tensor()
    dims, rank = capi.dims_arr((n,))
    assert L.to_wrap(y.ptr, capi.TO_F32, rank, dims, n_idx, C.byref(alias)) == 0
    assert call(ll=alias.value) == ARG                                           # losses aliased to Y
    L.to_release(alias)
    assert call(nn=None) == ARG                                                  # no lengths
    assert 2 not in idx                                                          # (sequence 2 is one idx does not name)
    assert call(nn=[5, 1, 0, 2, 4, 1]) == SHAPE                                  # a length of 0, at a sequence idx never names
    assert call(nn=[5, 1, 3, n + 1, 4, 1]) == SHAPE                              # a length of T + 1
    assert call(nn=[5, -1, 3, 2, 4, 1]) == SHAPE                                 # a negative length
    with Graph():
        st = call()
    assert st == STATE                                                           # refused while a capture records
    assert same(all_bits(dl, losses), start)                                     # nothing was written
    assert np.array_equal(bits(y.numpy()), bits(Y))
    assert call() == 0
    ls = losses.numpy()
    assert all(not np.any(ls[j, :lens[q]] == dt(7.5)) and not bits(ls[j, lens[q]:]).any() for j, q in enumerate(idx))
    assert not same(all_bits(dl, None), start[:-1])


@pytest.mark.parametrize("dt", [F32, F64], ids=ident)
@pytest.mark.parametrize("mode", [0, 2], ids=["per_sequence", "persistent"])
def test_non_finite(Ts, dt, mode):
    """one NaN inside the valid steps of X[idx[1]]: the call returns, and the NaN pattern of parameters, states and losses is
    the restatement's -- nothing in the kernel masks or clamps it"""
    from tensor_ops_amd.hipt import HipT
    i, spec, out_act, n, N, idx, lens, _, (rs, rp), _ = CASES["mixed"]
    T = Ts[dt]
    layers, X, Y = data("mixed", dt)
    Xn = X.copy()
    assert lens[idx[1]] > 2
    Xn[idx[1], 2, 3] = np.nan
    with np.errstate(all="ignore"):
        want_layers, want_losses = ORN.online(layers, Xn, Y, lens, idx, rs, rp, "tanh", out_act)
    HipT.rnn_online_persistent(mode)
    dl = dev(T, layers)
    losses = T.rnn_stack_online_sgd_ragged(dl, T.put(Xn, batched=True), T.put(Y, batched=True), lens, rs, rp, idx=idx,
                                           out_act=out_act, loss=LOSS[out_act], hidden_act="tanh", want_losses=True)
    assert np.array_equal(np.isnan(losses.numpy()), np.isnan(want_losses))
    assert np.isnan(want_losses).any() and not np.isnan(want_losses).all()
    for l, want in enumerate(want_layers):
        for c in range(4):
            if want[c] is not None:
                assert np.array_equal(np.isnan(dl[l][c].numpy()), np.isnan(want[c])), (l, c)
