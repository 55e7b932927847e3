"""Minibatch BPTT on sequences of their own lengths in one call (to_rnn_stack_minibatch_sgd_ragged,
csrc/rnn_minibatch_ragged.hip): one to_rnn_stack_sgd_ragged update per M sequences of idx, on both routes
(to_set_rnn_minibatch_persistent 0: per minibatch, 2: the persistent kernel on packed rows wherever its plan exists).

Checked against the float64 restatement tests/rnn_minibatch_ragged_numpy.py (held to three older restatements by
tests/test_rnn_minibatch_ragged_numpy_ref.py).  Tolerance: tests/test_gpu_rnn_tanh.py's TOL times 5 (5e-5 / 5e-11 relative
l2), the project's bound for a chain of at most 5 updates; no case has more than 3.  The chains do not amplify: on the CPU, for
exactly these cases, seeds and draws and both hidden activations, the restatement with the parameters rounded to fp32 after
every update stays within 3.5e-7 of the unrounded one (relative l2, the worst tensor), parameters stay below 3.2 in magnitude and
every case moves every one of its parameter tensors by at least 0.4 % relative l2, eighty times the fp32 bound (longT, whose
rates its 200 steps keep small; the other cases move theirs by 1 % to 34 %).
Then: padding is never read and losses are +0.0 there, route A is the caller's own loop bit for bit, all lengths T give the
dense entry's bits on both routes, cutting and repeating a call give identical bits, the persistent route's launch count
depends on neither n_idx nor M nor the lengths, and the contract.

Measured on an MI355X (max over parameters, states and losses of the relative l2 error against the restatement, max over the
cases and hidden activations; printed by test_parity): route A 2.8e-7 in fp32 and 5.4e-16 in fp64, route B 4.5e-7 and 4.4e-16;
the bounds are 5e-5 and 5e-11."""
import ctypes as C
import functools

import numpy as np
import pytest

import rnn_minibatch_ragged_numpy as MR
from test_gpu_rnn_minibatch import all_bits, ident, same
from test_gpu_rnn_tanh import LOSS, TOL, dev, make, rel_err

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
MIXED = [(12, "tanh"), (9, "logistic"), (5, None)]
M17_LENS = [4, 3, 3, 3, 3] + [2] * 11 + [1, 2, 4, 1]   # the first 17: act(t) = 17, 16, 5, 1

# name: (i, [(n, state_act)], out_act, T, lens (one per sequence), idx, M, (rate_state, rate_params), dtypes with a plan)
CASES = {
    "mixed": (7, MIXED, "softmax", 5, [5, 2, 1, 3, 5, 4, 5, 1], [3, 0, 3, 5, 1, 7, 2], 3, (0.3, 0.1), [F32, F64]),
    "m17": (6, [(6, "tanh")], "logistic", 4, M17_LENS, list(range(17)) + [19, 18, 17, 3], 17, (0.2, 0.1), [F32, F64]),
    "len1": (7, MIXED, "softmax", 3, [1] * 6, [0, 1, 2, 3, 4, 5, 1], 4, (0.5, 0.3), [F32, F64]),
    "m16_wide": (70, [(130, "logistic"), (3, None)], "softmax", 3, [3, 1, 2, 2] * 4, list(range(16)) + list(range(15, -1, -1)),
                 16, (0.3, 0.1), [F32]),
    "longT": (3, [(4, "tanh"), (3, None)], "softmax", 200, [200, 37, 1, 200, 37], [1, 0, 4, 2, 3, 1, 0], 4, (0.02, 0.005),
              [F32, F64]),
}
ALL_T = {"mixed": [3, 0, 3, 5, 1, 7], "m17": (list(range(20)) + list(range(19, 5, -1)))}   # n_idx a multiple of M


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
def data(name, dt, pad="random"):
    """the case's layers, X and Y; pad: what the rows t >= lens[q] hold"""
    i, spec, _, T, lens = CASES[name][:5]
    rng = np.random.default_rng(0x72 + T + len(lens) + len(name))
    layers = make(rng, i, spec, dt)
    X, Y = rng.uniform(-1, 1, (len(lens), T, i)).astype(dt), rng.uniform(0.1, 0.9, (len(lens), T, spec[-1][0])).astype(dt)
    for q, n in enumerate(lens):
        if pad == "nan":
            X[q, n:], Y[q, n:] = np.nan, np.nan
    return layers, X, Y


@functools.lru_cache(maxsize=None)
def reference(name, dt, hidden):
    """computed once per (case, dtype, hidden activation) and shared; nobody writes to it"""
    layers, X, Y = data(name, dt)
    _, _, out_act, _, lens, idx, M, (rs, rp), _ = CASES[name]
    return MR.minibatch(layers, X, Y, lens, idx, M, rs, rp, hidden, out_act)


def run(T, name, dl, x, y, idx=None, hidden="tanh", M=None, lens=None, losses=True):
    _, _, out_act, _, lens0, idx0, M0, (rs, rp), _ = CASES[name]
    return T.rnn_stack_minibatch_sgd_ragged(dl, x, y, lens or lens0, rs, rp, M or M0, idx=idx0 if idx is None else idx,
                                            out_act=out_act, loss=LOSS[out_act], hidden_act=hidden, want_losses=losses)


def put(T, name, dt, pad="random"):
    layers, X, Y = data(name, dt, pad)
    return layers, T.put(X, batched=True), T.put(Y, batched=True)


@pytest.mark.parametrize("name,dt,hidden,mode", [(n, dt, h, m) for n in CASES for dt in (F32, F64) for h in ("tanh", "logistic")
                                                 for m in (0, 2)], ids=ident)
def test_parity(Ts, name, dt, hidden, mode):
    from tensor_ops_amd.hipt import HipT
    T = Ts[dt]
    layers, x, y = put(T, name, dt)
    want_layers, want_losses = reference(name, dt, hidden)
    HipT.rnn_minibatch_persistent(mode)
    dl = dev(T, layers)
    p0, d0 = HipT.rnn_minibatch_ragged_stats(), HipT.rnn_minibatch_stats()
    losses = run(T, name, dl, x, y, hidden=hidden)
    p1 = HipT.rnn_minibatch_ragged_stats()
    assert (p1[0] - p0[0], p1[1] - p0[1]) == ((1, 0) if mode == 2 and dt in CASES[name][8] else (0, 1))
    assert HipT.rnn_minibatch_stats() == d0   # the dense entry's counters do not move
    errs = [rel_err(losses.numpy(), want_losses)]
    for l, want in enumerate(want_layers):
        errs += [rel_err(dl[l][c].numpy(), want[c]) for c in range(4) if want[c] is not None]
    print(name, ident(dt), hidden, "mode", mode, "max error", max(errs))
    assert max(errs) < 5 * TOL[dt]


@pytest.mark.parametrize("mode", [0, 2], ids=["per_minibatch", "persistent"])
@pytest.mark.parametrize("name", list(CASES))
def test_padding_is_never_read(Ts, name, mode):
    from tensor_ops_amd.hipt import HipT
    T = Ts[F32]
    HipT.rnn_minibatch_persistent(mode)
    got = []
    for pad in ("random", "nan"):
        layers, x, y = put(T, name, F32, pad)
        dl = dev(T, layers)
        got.append(all_bits(dl, run(T, name, dl, x, y)))
    assert same(got[0], got[1])
    lens, idx = CASES[name][4:6]
    pad = np.arange(CASES[name][3])[None, :] >= np.array([lens[q] for q in idx])[:, None]
    assert not got[0][-1][pad].any() and got[0][-1][~pad].all()   # +0.0, sign bit clear, exactly at the padding


@pytest.mark.parametrize("dt", [F32, F64], ids=ident)
@pytest.mark.parametrize("name", ["mixed", "m17"])
def test_route_a_is_the_callers_loop(Ts, name, dt):
    """mode 0: bit for bit a Python loop of batch_gather + rnn_stack_sgd with the gathered lengths"""
    from tensor_ops_amd.hipt import HipT
    _, _, out_act, _, lens, idx, M, (rs, rp), _ = CASES[name]
    T = Ts[dt]
    layers, x, y = put(T, name, dt)
    HipT.rnn_minibatch_persistent(0)
    dl, dl2, rows = dev(T, layers), dev(T, layers), []
    losses = run(T, name, dl, x, y)
    for k in range(0, len(idx), M):
        q = idx[k:k + M]
        rows.append(T.rnn_stack_sgd(dl2, T.batch_gather(x, q), T.batch_gather(y, q), rs, rp, out_act, LOSS[out_act],
                                    want_losses=True, hidden_act="tanh", lens=[lens[s] for s in q]).numpy())
    assert same(all_bits(dl, losses), all_bits(dl2, np.concatenate(rows)))


@pytest.mark.parametrize("mode", [0, 2], ids=["per_minibatch", "persistent"])
@pytest.mark.parametrize("name", list(ALL_T))
def test_all_lengths_T_is_the_dense_entry(Ts, name, mode):
    from tensor_ops_amd.hipt import HipT
    _, _, out_act, n, lens, _, M, (rs, rp), _ = CASES[name]
    T = Ts[F32]
    layers, x, y = put(T, name, F32)
    HipT.rnn_minibatch_persistent(mode)
    dl, dl2 = dev(T, layers), dev(T, layers)
    got = run(T, name, dl, x, y, idx=ALL_T[name], lens=[n] * len(lens))
    want = T.rnn_stack_minibatch_sgd(dl2, x, y, rs, rp, M, idx=ALL_T[name], out_act=out_act, loss=LOSS[out_act],
                                     hidden_act="tanh", want_losses=True)
    assert same(all_bits(dl, got), all_bits(dl2, want))


@pytest.mark.parametrize("mode", [0, 2], ids=["per_minibatch", "persistent"])
@pytest.mark.parametrize("name", ["mixed", "m17"])
def test_cut_and_repeat(Ts, name, mode):
    from tensor_ops_amd.hipt import HipT
    idx, M = CASES[name][5:7]
    T = Ts[F32]
    layers, x, y = put(T, name, F32)
    HipT.rnn_minibatch_persistent(mode)
    whole, again, cut = dev(T, layers), dev(T, layers), dev(T, layers)
    lw, la = run(T, name, whole, x, y), run(T, name, again, x, y)
    assert same(all_bits(whole, lw), all_bits(again, la))
    l1, l2 = run(T, name, cut, x, y, idx=idx[:M]), run(T, name, cut, x, y, idx=idx[M:])
    assert same(all_bits(whole, lw), all_bits(cut, np.concatenate([l1.numpy(), l2.numpy()])))
    assert not same(all_bits(whole, None), all_bits(dev(T, layers), None))   # (something was trained)


def test_launch_count(Ts):
    """mode 2: the launches of a call depend on neither n_idx nor M nor the lengths"""
    from tensor_ops_amd.hipt import HipT
    T = Ts[F32]
    HipT.rnn_minibatch_persistent(2)
    layers, x, y = put(T, "mixed", F32)
    idx = CASES["mixed"][5]

    def launches(idx, M=None, lens=None):
        dl = dev(T, layers)
        l0 = T.stats()["launches"]
        run(T, "mixed", dl, x, y, idx=idx, M=M, lens=lens, losses=False)
        return T.stats()["launches"] - l0
    launches(idx)   # (a process's first call: the kernel's attribute, the pool)
    counts = [launches(idx), launches(idx + idx, M=5, lens=[1, 5, 2, 2, 4, 1, 3, 5])]
    assert counts[0] == counts[1], counts


@pytest.mark.parametrize("mode", [0, 2], ids=["per_minibatch", "persistent"])
def test_contract(Ts, mode):
    from tensor_ops_amd import capi
    from tensor_ops_amd.hipt import Graph, HipT
    L = capi.lib()
    T, dt = Ts[F32], F32
    _, _, _, n, lens, idx, M, (rs, rp), _ = CASES["mixed"]
    layers, x, y = put(T, "mixed", dt)
    dl = dev(T, layers)
    losses = T.put(np.full((len(idx), n), 7.5, dt), batched=True)
    start = all_bits(dl, losses)
    ARG, SHAPE, STATE = 1, 2, 4
    HipT.rnn_minibatch_persistent(mode)
    d0 = HipT.rnn_minibatch_stats()

    def call(ll=lens, ii=idx, m=M, ls=losses.h):
        arr = lambda c: (capi.c_tensor * 3)(*[(lay[c].h if lay[c] is not None else None) for lay in dl])  # noqa: E731
        ia, la = np.ascontiguousarray(ii, np.int64), None if ll is None else np.ascontiguousarray(ll, np.int64)
        return L.to_rnn_stack_minibatch_sgd_ragged(3, (C.c_int * 3)(3, 0, -1), arr(0), arr(1), arr(2), arr(3), 0, 2, 1, x.h, y.h,
                                                   None if la is None else la.ctypes.data_as(C.POINTER(C.c_int64)), len(ii),
                                                   ia.ctypes.data_as(C.POINTER(C.c_int64)), m, rs, rp, ls)
    assert call(ll=None) == ARG and call(m=0) == ARG
    for seq in (3, 4):   # (idx names 3, never 4)
        assert call(ll=lens[:seq] + [0] + lens[seq + 1:]) == SHAPE and call(ll=lens[:seq] + [n + 1] + lens[seq + 1:]) == SHAPE
    assert call(ii=[3, 0, len(lens), 5, 1, 7, 2]) == SHAPE        # an index = N
    alias = capi.c_tensor()                                        # losses overlapping X
    dims, rank = capi.dims_arr((n,))
    assert L.to_wrap(x.ptr, capi.TO_F32, rank, dims, len(idx), C.byref(alias)) == 0
    assert call(ls=alias.value) == ARG
    L.to_release(alias)
    with Graph():
        st = call()
    assert st == STATE                                             # refused while a capture records
    assert same(all_bits(dl, losses), start)                       # nothing was written
    assert call() == 0 and not same(all_bits(dl, losses), start)
    assert HipT.rnn_minibatch_stats() == d0
