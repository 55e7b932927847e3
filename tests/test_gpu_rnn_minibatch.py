"""Minibatch BPTT in one call (to_rnn_stack_minibatch_sgd, csrc/rnn_minibatch.hip): one to_rnn_stack_sgd update per M sequences
of idx, on both routes (to_set_rnn_minibatch_persistent 0: per minibatch, 2: the persistent MFMA kernel wherever its plan exists).

Checked against the float64 restatement tests/rnn_minibatch_numpy.py (held to tests/rnn_online_numpy.py and act_numpy's BPTT
by tests/test_rnn_minibatch_numpy_ref.py).  Tolerance: tests/test_gpu_rnn_tanh.py's TOL times 5 (5e-5 / 5e-11 relative l2), the
bound tests/test_gpu_rnn_online.py uses for a chain of at most 5 updates.  The chains do not amplify: on the CPU, for exactly
these cases, seeds and draws and both hidden activations, the restatement with the parameters rounded to fp32 after every
update stays within 8e-8 of the unrounded one, parameters stay below 1.7 in magnitude, everything is finite and every case moves
its parameters by at least 9 % relative l2.  Then: route A is the caller's own loop bit for bit, cutting a call at a minibatch
boundary and repeating a call give identical bits on both routes, the launch count of the persistent route depends on neither
n_idx nor M nor T, and the contract.

Measured on an MI355X (max over parameters, states and losses of the relative l2 error against the restatement, max over the
cases and hidden activations; printed by test_parity): route A 9.7e-8 in fp32 and 4.2e-16 in fp64, route B 1.1e-7 and 3.9e-16;
the bounds are 5e-5 and 5e-11."""
import ctypes as C
import functools

import numpy as np
import pytest

import rnn_minibatch_numpy as MN
from test_gpu_rnn_tanh import LOSS, TOL, dev, make, rel_err

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
UPDOWN = lambda n, lo: list(range(n)) + list(range(n - 1, lo - 1, -1))  # noqa: E731
MIXED = [(12, "tanh"), (9, "logistic"), (5, None)]

# name: (i, [(n, state_act)], out_act, T, N, idx, M, (rate_state, rate_params), dtypes with a plan)
CASES = {
    "mixed": (7, MIXED, "softmax", 5, 8, [3, 0, 3, 5, 1, 7, 2], 3, (0.1, 0.02), [F32, F64]),
    "T1": (7, MIXED, "softmax", 1, 4, [2, 0, 1, 3, 3], 2, (0.1, 0.02), [F32, F64]),
    "m17": (6, [(6, "tanh")], "logistic", 4, 20, UPDOWN(20, 1), 17, (0.02, 0.005), [F32, F64]),
    "m16_wide": (70, [(130, "logistic"), (3, None)], "softmax", 3, 16, UPDOWN(16, 0), 16, (0.02, 0.005), [F32]),
    "longT": (3, [(4, "tanh"), (3, None)], "softmax", 200, 5, [1, 0, 4, 2, 3, 1, 0], 4, (0.003, 0.0005), [F32, F64]),
    "m1": (6, [(6, "tanh")], "logistic", 4, 4, [1, 1, 3, 0], 1, (0.3, 0.05), [F32, F64]),
}


@pytest.fixture(scope="module")
def Ts():
    from tensor_ops_amd.hipt import HipT
    return {F32: HipT(0, F32), F64: HipT(0, F64)}


@pytest.fixture(autouse=True)
def auto_route():
    from tensor_ops_amd.hipt import HipT
    prev = HipT.rnn_minibatch_persistent(1)
    yield
    HipT.rnn_minibatch_persistent(prev)


@functools.lru_cache(maxsize=None)
def data(name, dt, T=None):
    i, spec, _, T0, N = CASES[name][:5]
    T = T or T0
    rng = np.random.default_rng(0x71 + T + N + len(name))
    layers = make(rng, i, spec, dt)
    return layers, rng.uniform(-1, 1, (N, T, i)).astype(dt), rng.uniform(0.1, 0.9, (N, T, spec[-1][0])).astype(dt)


@functools.lru_cache(maxsize=None)
def reference(name, dt, hidden):
    """computed once per (case, dtype, hidden activation) and shared; nobody writes to it"""
    layers, X, Y = data(name, dt)
    _, _, out_act, _, _, idx, M, (rs, rp), _ = CASES[name]
    return MN.minibatch(layers, X, Y, idx, M, rs, rp, hidden, out_act)


def run(T, name, dl, x, y, idx="case", hidden="tanh", M=None, losses=True):
    _, _, out_act, _, _, idx0, M0, (rs, rp), _ = CASES[name]
    return T.rnn_stack_minibatch_sgd(dl, x, y, rs, rp, M or M0, idx=idx0 if isinstance(idx, str) else idx, out_act=out_act,
                                     loss=LOSS[out_act], hidden_act=hidden, want_losses=losses)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def all_bits(dl, losses):
    out = [bits(t.numpy()) for lay in dl for t in lay[:4] if t is not None]
    return out + ([bits(losses if isinstance(losses, np.ndarray) else losses.numpy())] if losses is not None else [])


def same(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b))


def ident(v):
    return getattr(v, "__name__", str(v))


@pytest.mark.parametrize("name,dt,hidden,mode", [(n, dt, h, m) for n in CASES for dt in (F32, F64) for h in ("tanh", "logistic")
                                                 for m in (0, 2)], ids=ident)
def test_parity(Ts, name, dt, hidden, mode):
    from tensor_ops_amd.hipt import HipT
    T = Ts[dt]
    layers, X, Y = data(name, dt)
    want_layers, want_losses = reference(name, dt, hidden)
    HipT.rnn_minibatch_persistent(mode)
    dl = dev(T, layers)
    p0 = HipT.rnn_minibatch_stats()
    losses = run(T, name, dl, T.put(X, batched=True), T.put(Y, batched=True), hidden=hidden)
    p1 = HipT.rnn_minibatch_stats()
    assert (p1[0] - p0[0], p1[1] - p0[1]) == ((1, 0) if mode == 2 and dt in CASES[name][8] else (0, 1))
    errs = [rel_err(losses.numpy(), want_losses)]
    for l, want in enumerate(want_layers):
        errs += [rel_err(dl[l][c].numpy(), want[c]) for c in range(4) if want[c] is not None]
        assert want[1] is not None or (dl[l][0] is None and dl[l][1] is None)
    print(name, ident(dt), hidden, "mode", mode, "max error", max(errs))
    assert max(errs) < 5 * TOL[dt]


@pytest.mark.parametrize("dt", [F32, F64], ids=ident)
@pytest.mark.parametrize("name", ["mixed", "m17", "m1"])
def test_route_a_is_the_callers_loop(Ts, name, dt):
    """mode 0: bit for bit a Python loop of batch_gather + rnn_stack_sgd; at M = 1 also rnn_stack_online_sgd's route A"""
    from tensor_ops_amd.hipt import HipT
    _, _, out_act, _, _, idx, M, (rs, rp), _ = CASES[name]
    T = Ts[dt]
    layers, X, Y = data(name, dt)
    x, y = T.put(X, batched=True), T.put(Y, batched=True)
    HipT.rnn_minibatch_persistent(0)
    dl = dev(T, layers)
    losses = run(T, name, dl, x, y)
    dl2, rows = dev(T, layers), []
    if name == "m1":
        prev = HipT.rnn_online_persistent(0)
        rows = [T.rnn_stack_online_sgd(dl2, x, y, rs, rp, idx=idx, out_act=out_act, loss=LOSS[out_act], hidden_act="tanh",
                                       want_losses=True).numpy()]
        HipT.rnn_online_persistent(prev)
    for k in range(0, len(idx) if name != "m1" else 0, M):
        q = idx[k:k + M]
        rows.append(T.rnn_stack_sgd(dl2, T.batch_gather(x, q), T.batch_gather(y, q), rs, rp, out_act, LOSS[out_act],
                                    want_losses=True, hidden_act="tanh").numpy())
    assert same(all_bits(dl, losses), all_bits(dl2, np.concatenate(rows)))


@pytest.mark.parametrize("mode", [0, 2], ids=["per_minibatch", "persistent"])
@pytest.mark.parametrize("name", ["mixed", "m17"])
def test_cut_and_repeat(Ts, name, mode):
    from tensor_ops_amd.hipt import HipT
    idx, M = CASES[name][5:7]
    T = Ts[F32]
    layers, X, Y = data(name, F32)
    x, y = T.put(X, batched=True), T.put(Y, batched=True)
    HipT.rnn_minibatch_persistent(mode)
    whole, again, cut = dev(T, layers), dev(T, layers), dev(T, layers)
    lw, la = run(T, name, whole, x, y), run(T, name, again, x, y)
    assert same(all_bits(whole, lw), all_bits(again, la))
    l1, l2 = run(T, name, cut, x, y, idx=idx[:M]), run(T, name, cut, x, y, idx=idx[M:])
    assert same(all_bits(whole, lw), all_bits(cut, np.concatenate([l1.numpy(), l2.numpy()])))
    assert not same(all_bits(whole, None), all_bits(dev(T, layers), None))   # (something was trained)


def test_launch_count(Ts):
    """mode 2: the launches of a call depend on neither n_idx nor M nor T"""
    from tensor_ops_amd.hipt import HipT
    T = Ts[F32]
    HipT.rnn_minibatch_persistent(2)

    def launches(name, idx, M=None, steps=None):
        layers, X, Y = data(name, F32, steps)
        x, y, dl = T.put(X, batched=True), T.put(Y, batched=True), dev(T, layers)
        l0 = T.stats()["launches"]
        run(T, name, dl, x, y, idx=idx, M=M, losses=False)
        return T.stats()["launches"] - l0
    idx = CASES["mixed"][5]
    launches("mixed", idx)   # (a process's first call: the kernel's attribute, the pool)
    counts = [launches("mixed", idx), launches("mixed", idx + idx), launches("mixed", idx, M=5),
              launches("longT", CASES["longT"][5]), launches("longT", CASES["longT"][5], steps=5)]
    assert counts[0] == counts[1] == counts[2] and counts[3] == counts[4], counts


@pytest.mark.parametrize("mode", [0, 2], ids=["per_minibatch", "persistent"])
def test_contract(Ts, mode):
    from tensor_ops_amd import capi
    from tensor_ops_amd.hipt import Graph, HipT
    L = capi.lib()
    T, dt = Ts[F32], F32
    _, _, _, n, N, idx, M, (rs, rp), _ = CASES["mixed"]
    layers, X, Y = data("mixed", dt)
    dl = dev(T, layers)
    x, y = T.put(X, batched=True), T.put(Y, batched=True)
    losses = T.put(np.full((len(idx), n), 7.5, dt), batched=True)
    start = all_bits(dl, losses)
    ARG, SHAPE, STATE, UNSUPPORTED = 1, 2, 4, 5
    HipT.rnn_minibatch_persistent(mode)

    def call(xx=x, k=len(idx), ii=idx, m=M, out_act_=2):
        arr = lambda c: (capi.c_tensor * 3)(*[(lay[c].h if lay[c] is not None else None) for lay in dl])  # noqa: E731
        ia = np.ascontiguousarray(ii, np.int64)
        return L.to_rnn_stack_minibatch_sgd(3, (C.c_int * 3)(3, 0, -1), arr(0), arr(1), arr(2), arr(3), 0, out_act_, 1, xx.h, y.h,
                                            k, ia.ctypes.data_as(C.POINTER(C.c_int64)), m, rs, rp, losses.h)
    assert call(m=0) == ARG and call(k=0) == ARG
    assert call(ii=[3, 0, N, 5, 1, 7, 2]) == SHAPE                 # an index = N
    assert call(out_act_=3) == UNSUPPORTED                         # tanh as out_act
    with Graph():
        st = call()
    assert st == STATE                                             # refused while a capture records
    assert same(all_bits(dl, losses), start)                       # nothing was written
    # NaN in a sequence idx never names (4, 6) changes no bit; NaN in idx[3] = 5: the second update's parameters are NaN, the
    # first minibatch's losses finite and unchanged
    assert call() == 0
    clean = all_bits(dl, losses)
    for seq, poisoned in ((4, False), (6, False), (5, True)):
        Xn = X.copy()
        Xn[seq] = np.nan
        dl = dev(T, layers)
        assert call(xx=T.put(Xn, batched=True)) == 0
        got = all_bits(dl, losses)
        if not poisoned:
            assert same(got, clean)
        else:
            assert np.isnan(dl[0][2].numpy()).all() and np.array_equal(got[-1][:M], clean[-1][:M])
            assert np.isfinite(losses.numpy()[:M]).all()
    assert L.to_set_rnn_minibatch_persistent(3, None) == ARG
