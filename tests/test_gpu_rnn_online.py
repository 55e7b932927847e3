"""Per-sequence training in one call (to_rnn_stack_online_sgd, csrc/rnn_online.hip): `trainNetwork'` folded over the sequences
idx[0 .. n_idx) of a resident set, every step from the parameters and the learned initial states the step before left, on
both routes (to_set_rnn_online_persistent 0: per sequence, 2: the persistent kernel, 1: automatic).

Checked against the float64 restatement tests/rnn_online_numpy.py (held to oracle/recurrent.py's trainNetwork at 1e-10 by
tests/test_rnn_online_numpy_ref.py).  Tolerance: tests/test_gpu_rnn_tanh.py's TOL (1e-5 / 1e-11 relative l2) times its
factor 5, here for a chain of at most 5 updates.  The chains do not amplify: on the CPU, for these cases, the restatement with
the parameters rounded to fp32 after every update stays within 9e-8 of the unrounded one, the parameters stay below 1.6 in
magnitude and everything is finite.  Then: route A is the caller's own loop bit for bit, cutting a chain into two calls and
repeating a call give identical bits on both routes, the launch count of the persistent route depends neither on n_idx nor
on T, a stack beyond the kernel's LDS runs per sequence, the contract, and a NaN in one sequence.

Measured on an MI355X (max over parameters, states and losses of the relative l2 error against the restatement, max over
the cases and hidden activations; printed by test_parity): route A 1.4e-7 in fp32 and 8.5e-16 in fp64, route B 3.0e-7 and
4.7e-16; the bounds are 5e-5 and 5e-11."""
import ctypes as C
import functools

import numpy as np
import pytest

import rnn_online_numpy as ON
from test_gpu_rnn_tanh import LOSS, TOL, dev, make, rel_err

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
H_STAR = 128   # include/tensorops_hip.h: automatic = route B where the plan fits and no layer is wider

# name: (i, [(n, state_act)], out_act, T, N, idx, dtypes, (rate_state, rate_params), dtypes whose plan fits the kernel's LDS)
CASES = {
    "mixed": (7, [(12, "tanh"), (9, "logistic"), (5, None)], "softmax", 5, 6, [3, 0, 3, 5, 1], [F32, F64], (0.3, 0.05), [F32, F64]),
    # no recurrence in the backward; gs still flows
    "T1": (7, [(12, "tanh"), (9, "logistic"), (5, None)], "softmax", 1, 3, [2, 0, 1], [F32, F64], (0.3, 0.05), [F32, F64]),
    # a stateful output layer under the logistic head, and an immediate repeat
    "state_head": (6, [(6, "tanh")], "logistic", 4, 4, [1, 1, 3, 0], [F32, F64], (0.3, 0.05), [F32, F64]),
    # widths above 64 and 128 that are no multiples of 64; in fp64 the parameters exceed the LDS: no plan
    "wide": (70, [(130, "logistic"), (3, None)], "softmax", 3, 3, [0, 2, 1], [F32, F64], (0.3, 0.05), [F32]),
    # T does not bound the range, whichever home the tape takes: here 600 records of 18 elements, 43 KB (fp32) / 86 KB (fp64),
    # in LDS beside the parameters
    "longT": (3, [(4, "tanh"), (3, None)], "softmax", 600, 2, [1, 0, 1], [F32, F64], (0.01, 0.002), [F32, F64]),
    # ... and the other home: in fp32 the parameters, states and rows take 107 KiB of the 160 and leave room for 28 records of
    # 472 elements; the tape's 40 records (74 KiB) are in global memory
    "wide_T40": (70, [(130, "logistic"), (3, None)], "softmax", 40, 2, [1, 0, 1], [F32], (0.01, 0.002), [F32]),
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
    i, spec, out_act, T, N, idx, _, _, _ = CASES[name]
    rng = np.random.default_rng(0x61 + T + N + len(name))
    layers = make(rng, i, spec, dt)
    X = rng.uniform(-1, 1, (N, T, i)).astype(dt)
    Y = rng.uniform(0.1, 0.9, (N, T, spec[-1][0])).astype(dt)
    return layers, X, Y


@functools.lru_cache(maxsize=None)
def reference(name, dt, hidden):
    """computed once per (case, dtype, hidden activation) and shared; nobody writes to it"""
    layers, X, Y = data(name, dt)
    out_act, idx, rates = CASES[name][2], CASES[name][5], CASES[name][7]
    return ON.online(layers, X, Y, idx, rates[0], rates[1], hidden, out_act)


def expect_persistent(name, dt, mode):
    spec, fits = CASES[name][1], dt in CASES[name][8]
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


PARITY = [(name, dt, hidden, mode) for name, c in CASES.items() for dt in c[6] for hidden in ("tanh", "logistic")
          for mode in (0, 1, 2)]


def ident(v):
    return getattr(v, "__name__", str(v))


@pytest.mark.parametrize("name,dt,hidden,mode", PARITY, ids=ident)
def test_parity(Ts, name, dt, hidden, mode):
    from tensor_ops_amd.hipt import HipT
    i, spec, out_act, n, N, idx, _, (rs, rp), _ = CASES[name]
    T = Ts[dt]
    layers, X, Y = data(name, dt)
    want_layers, want_losses = reference(name, dt, hidden)
    HipT.rnn_online_persistent(mode)
    dl = dev(T, layers)
    p0 = HipT.rnn_online_stats()
    losses = T.rnn_stack_online_sgd(dl, T.put(X, batched=True), T.put(Y, batched=True), rs, rp, idx=idx, out_act=out_act,
                                    loss=LOSS[out_act], hidden_act=hidden, want_losses=True)
    p1 = HipT.rnn_online_stats()
    assert (p1[0] - p0[0], p1[1] - p0[1]) == ((1, 0) if expect_persistent(name, dt, mode) else (0, 1))
    assert losses.numpy().shape == (len(idx), n)
    errs = errors(dl, losses, want_layers, want_losses)
    print(name, ident(dt), hidden, "mode", mode, "max error", max(errs))
    assert max(errs) < 5 * TOL[dt]


@pytest.mark.parametrize("dt", [F32, F64], ids=ident)
@pytest.mark.parametrize("name", ["mixed", "state_head"])
def test_route_a_is_the_callers_loop(Ts, name, dt):
    """mode 0: bit for bit a Python loop of rnn_stack_sgd over batch_select views of the same device X / Y"""
    from tensor_ops_amd.hipt import HipT
    i, spec, out_act, n, N, idx, _, (rs, rp), _ = CASES[name]
    T = Ts[dt]
    layers, X, Y = data(name, dt)
    x, y = T.put(X, batched=True), T.put(Y, batched=True)
    HipT.rnn_online_persistent(0)
    for hidden in ("tanh", "logistic"):
        dl = dev(T, layers)
        losses = T.rnn_stack_online_sgd(dl, x, y, rs, rp, idx=idx, out_act=out_act, loss=LOSS[out_act], hidden_act=hidden,
                                        want_losses=True)
        dl2, rows = dev(T, layers), []
        for q in idx:
            ls = T.rnn_stack_sgd(dl2, T.batch_select(x, q), T.batch_select(y, q), rs, rp, out_act, LOSS[out_act],
                                 want_losses=True, hidden_act=hidden)
            rows.append(ls.numpy())
        assert same(all_bits(dl, None), all_bits(dl2, None))
        assert np.array_equal(bits(losses.numpy()), bits(np.stack(rows)))


@pytest.mark.parametrize("dt", [F32, F64], ids=ident)
@pytest.mark.parametrize("mode", [0, 2], ids=["per_sequence", "persistent"])
def test_cutting_and_determinism(Ts, dt, mode):
    from tensor_ops_amd.hipt import HipT
    i, spec, out_act, n, N, idx, _, (rs, rp), _ = CASES["mixed"]
    T = Ts[dt]
    layers, X, Y = data("mixed", dt)
    x, y = T.put(X, batched=True), T.put(Y, batched=True)
    HipT.rnn_online_persistent(mode)

    def run(dl, ii, n_idx=None):
        return T.rnn_stack_online_sgd(dl, x, y, rs, rp, idx=ii, n_idx=n_idx, out_act=out_act, loss=LOSS[out_act],
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

    def launches(n_idx, n):
        X = rng.uniform(-1, 1, (6, n, i)).astype(dt)
        Y = rng.uniform(0.1, 0.9, (6, n, spec[-1][0])).astype(dt)
        x, y, dl = T.put(X, batched=True), T.put(Y, batched=True), dev(T, layers)
        idx = np.arange(n_idx) % 6
        T.rnn_stack_online_sgd(dl, x, y, 0.3, 0.05, idx=idx, out_act=out_act)
        l0 = T.stats()["launches"]
        T.rnn_stack_online_sgd(dl, x, y, 0.3, 0.05, idx=idx, out_act=out_act)
        return T.stats()["launches"] - l0
    HipT.rnn_online_persistent(2)
    a, b = launches(2, 3), launches(7, 9)
    assert a == b, (a, b)
    HipT.rnn_online_persistent(0)
    assert launches(2, 3) < launches(7, 3)   # the per-sequence route grows with n_idx


def test_out_of_range(Ts):
    """fp32 64 -> 160 (tanh) -> 64: 182 KiB of parameters, no plan: per sequence even when route B is forced -- and right"""
    from tensor_ops_amd.hipt import HipT
    T, dt = Ts[F32], F32
    rng = np.random.default_rng(0x33)
    layers = make(rng, 64, [(160, "tanh"), (64, None)], dt)
    X = rng.uniform(-1, 1, (2, 2, 64)).astype(dt)
    Y = rng.uniform(0.1, 0.9, (2, 2, 64)).astype(dt)
    idx = [1, 0]
    want_layers, want_losses = ON.online(layers, X, Y, idx, 0.3, 0.05, "logistic", "softmax")
    HipT.rnn_online_persistent(2)
    dl = dev(T, layers)
    p0 = HipT.rnn_online_stats()
    losses = T.rnn_stack_online_sgd(dl, T.put(X, batched=True), T.put(Y, batched=True), 0.3, 0.05, idx=idx, want_losses=True)
    p1 = HipT.rnn_online_stats()
    assert (p1[0] - p0[0], p1[1] - p0[1]) == (0, 1)
    errs = errors(dl, losses, want_layers, want_losses)
    print("out of range: max error", max(errs))
    assert max(errs) < 5 * TOL[dt]


def test_contract(Ts):
    from tensor_ops_amd import capi
    from tensor_ops_amd.hipt import Graph, HipT
    L = capi.lib()
    T, dt = Ts[F32], F32
    i, spec, out_act, n, N, idx, _, (rs, rp), _ = CASES["mixed"]
    layers, X, Y = data("mixed", dt)
    dl = dev(T, layers)
    x, y = T.put(X, batched=True), T.put(Y, batched=True)
    n_idx = len(idx)
    sentinel = lambda *shape: T.put(np.full(shape, 7.5, dt), batched=True)  # noqa: E731
    losses = sentinel(n_idx, n)
    start = all_bits(dl, losses)
    ARG, SHAPE, STATE, UNSUPPORTED = 1, 2, 4, 5

    def call(layers_=dl, xx=x, yy=y, k=n_idx, ii=idx, out_act_=2, loss_=1, ll=losses, sact=(3, 0, -1)):
        nl = len(layers_)
        arr = lambda c: (capi.c_tensor * nl)(*[(lay[c].h if lay[c] is not None else None) for lay in layers_])  # noqa
        ia = np.ascontiguousarray(ii, np.int64) if ii is not None else None
        return L.to_rnn_stack_online_sgd(nl, (C.c_int * nl)(*sact), arr(0), arr(1), arr(2), arr(3), 0, out_act_, loss_,
                                         xx.h, yy.h, k, ia.ctypes.data_as(C.POINTER(C.c_int64)) if ia is not None else None,
                                         rs, rp, ll if isinstance(ll, (int, type(None))) else ll.h)
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
    with Graph():
        st = call()
    assert st == STATE                                                           # refused while a capture records
    assert same(all_bits(dl, losses), start)                                     # nothing was written
    assert np.array_equal(bits(y.numpy()), bits(Y))
    assert call() == 0
    assert not np.any(losses.numpy() == dt(7.5)) and not same(all_bits(dl, None), start[:-1])
    assert HipT.rnn_online_persistent(1) in (0, 1, 2) and L.to_set_rnn_online_persistent(3, None) == ARG


@pytest.mark.parametrize("dt", [F32, F64], ids=ident)
@pytest.mark.parametrize("mode", [0, 2], ids=["per_sequence", "persistent"])
def test_non_finite(Ts, dt, mode):
    """one NaN in X[idx[1]]: the call returns, and the NaN pattern of parameters, states and losses is the restatement's --
    nothing in the kernel masks or clamps it"""
    from tensor_ops_amd.hipt import HipT
    i, spec, out_act, n, N, idx, _, (rs, rp), _ = CASES["mixed"]
    T = Ts[dt]
    layers, X, Y = data("mixed", dt)
    Xn = X.copy()
    Xn[idx[1], 2, 3] = np.nan
    with np.errstate(all="ignore"):
        want_layers, want_losses = ON.online(layers, Xn, Y, idx, rs, rp, "tanh", out_act)
    HipT.rnn_online_persistent(mode)
    dl = dev(T, layers)
    losses = T.rnn_stack_online_sgd(dl, T.put(Xn, batched=True), T.put(Y, batched=True), rs, rp, idx=idx, out_act=out_act,
                                    loss=LOSS[out_act], hidden_act="tanh", want_losses=True)
    assert np.array_equal(np.isnan(losses.numpy()), np.isnan(want_losses))
    assert np.isnan(want_losses).any() and not np.isnan(want_losses).all()
    for l, want in enumerate(want_layers):
        for c in range(4):
            if want[c] is not None:
                assert np.array_equal(np.isnan(dl[l][c].numpy()), np.isnan(want[c])), (l, c)
