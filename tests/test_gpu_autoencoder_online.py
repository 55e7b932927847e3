"""to_autoencoder_stack_online_sgd: `trainEncoder` folded over rows of a resident data set in one call, on both routes
(to_set_autoencoder_online_persistent 0: per sample, 2: the persistent kernel csrc/ae_online.hip).

Reference: a loop of tests/autoencoder_numpy.py's `sgd` on one row at a time in float64, from the parameters and rows as
stored in the element type under test, the per-row loss from its `run`.  Tolerance: RTOL of tests/test_gpu_autoencoder.py
(relative l2 1e-5 / 1e-11) times the chain length 5, as tests/test_gpu_rnn_online.py; losses through loss_err.  The chains do
not amplify: on the CPU, for every parity case, the restatement with the parameters rounded to fp32 after every update stays
within 1.3e-7 (relative l2, worst parameter) and 4.1e-8 (losses) of the unrounded one -- 400 times inside the bound of 5e-5 --
and no parameter exceeds 2.5 in magnitude.

Measured on an MI355X (worst parity case, max over parameters and losses; printed by test_parity): route A 1.7e-7 in fp32
and 3.3e-16 in fp64, route B 1.6e-7 and 3.3e-16; the bounds are 5e-5 and 5e-11.

Shapes are the smallest at which the partition can go wrong; see PLANS.  idx has a repeat and two equal consecutive
entries.  Cases with G > 1 skip only where the plan query says the placement probe failed; G = 1 and route A run anywhere."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest

import autoencoder_numpy as AEN
from test_gpu_autoencoder import RTOL, ident, loss_err, params, problem, put_net, rel_err, same_bits

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
N, IDX, RATE = 4, (2, 0, 2, 3, 3), 0.03   # (at 0.1 the all-identity [13, 7, 13] chain diverges: losses 24 -> 5e4)
OK, ARG, SHAPE, STATE, UNSUPPORTED = 0, 1, 2, 4, 5
# sizes: (n_enc, groups asked for, the plan: G, rows of layer 1 a workgroup, rows of layer L a workgroup)
PLANS = {
    (5, 3, 5): (1, 0, (1, 3, 0)),                 # L = 2, no second exchange, G = 1
    (13, 7, 13): (1, 3, (3, 3, 0)),               # uneven slices of layer 1: 3, 3, 1
    (13, 7, 4, 13): (2, 3, (3, 3, 5)),            # L = 3: the code layer is the exchanged layer 2; layer 3 in slices 5, 5, 3
    (13, 4, 7, 13): (1, 3, (4, 1, 4)),            # ... and the code layer is layer 1 (3 asked for: 4 rows make it 4 of one row)
    (12, 8, 5, 8, 12): (2, 4, (4, 2, 3)),         # one replicated layer
    (10, 8, 6, 4, 6, 10): (3, 2, (2, 4, 5)),      # two replicated layers
    (513, 2, 513): (1, 0, (1, 2, 0)),             # the second prefetch register of a thread
}
SMALL = [(5, 3, 5), (13, 7, 13)]
HEADS = ["logistic", "tanh", "identity"]          # the squaredError pairs
# (sizes, hidden, code_act, out_act): the product on the two smallest shapes, one combination on each of the others
PARITY = [(s, h, c, o) for s in SMALL for h, c, o in itertools.product(AEN.HIDDEN, AEN.CODE, HEADS)] + [
    ((13, 7, 4, 13), "tanh", "identity", "tanh"), ((13, 4, 7, 13), "logistic", "tanh", "identity"),
    ((12, 8, 5, 8, 12), "tanh", "logistic", "logistic"), ((10, 8, 6, 4, 6, 10), "logistic", "identity", "tanh"),
    ((513, 2, 513), "logistic", "logistic", "logistic")]


@pytest.fixture(scope="module")
def Ts():
    from tensor_ops_amd.hipt import HipT
    return {F32: HipT(0, F32), F64: HipT(0, F64)}


@pytest.fixture(autouse=True)
def settings():
    from tensor_ops_amd.hipt import HipT
    yield
    HipT.autoencoder_online_persistent(1)
    HipT.autoencoder_online_groups(0)


@functools.lru_cache(maxsize=None)
def case(sizes, dt, out_act):
    return problem(list(sizes), N, dt, 0xa0 + sum(sizes), out_act)


@functools.lru_cache(maxsize=None)
def reference(sizes, dt, hidden, code_act, out_act):
    """computed once per case and shared; nobody writes to it"""
    ws, X = case(sizes, dt, out_act)
    n_enc, losses = PLANS[sizes][0], []
    cur = [(w.astype(F64), b.astype(F64)) for w, b in ws]
    for q in IDX:
        losses.append(AEN.run(cur, n_enc, X[q:q + 1], hidden, code_act, out_act)[2][0])
        cur = AEN.sgd(cur, n_enc, X[q:q + 1], RATE, hidden, code_act, out_act)
    return [w for w, _ in cur] + [b for _, b in cur], np.array(losses)


def train(T, sizes, mode, hidden="logistic", code_act="logistic", out_act="logistic", idx=IDX, n=None, net=None, want=None):
    """one call on `mode`'s route from the case's parameters (or on the device parameters `net`); `want`: the (persistent,
    per sample) runs it must count.  Skips where a plan of several workgroups has no placement."""
    from tensor_ops_amd.hipt import HipT
    n_enc, groups, plan = PLANS[sizes]
    ws, X = case(sizes, T.dtype.type, out_act)
    HipT.autoencoder_online_persistent(mode)
    HipT.autoencoder_online_groups(groups)
    if mode == 2:
        got = T.autoencoder_online_plan(sizes)
        assert got["exists"] and (got["G"], got["slice_first"], got["slice_last"]) == plan, got
        assert got["grid"] == (1 if plan[0] == 1 else 8 * plan[0]) and got["lds_bytes"] <= 160 * 1024
        if plan[0] > 1 and not got["placement_ok"] and want is None:
            pytest.skip("workgroups b, b + 8, .. of a grid do not share an XCD on this device")
    W, b = net if net is not None else put_net(T, ws)
    s0 = HipT.autoencoder_online_stats()
    losses = T.autoencoder_online_sgd(W, b, n_enc, T.put(X, batched=True), RATE, idx=idx, n=n, out_act=out_act,
                                      loss=AEN.PAIRS[out_act], hidden_act=hidden, code_act=code_act, want_losses=True)
    s1 = HipT.autoencoder_online_stats()
    assert (s1[0] - s0[0], s1[1] - s0[1]) == (want or ((1, 0) if mode == 2 else (0, 1)))
    return (W, b), params(W, b) + [losses.numpy()]


def all_same(a, b):
    return len(a) == len(b) and all(same_bits(x, y) for x, y in zip(a, b))


# ---- 1. parity on both routes ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F32, F64], ids=ident)
@pytest.mark.parametrize("mode", [0, 2], ids=["per_sample", "persistent"])
@pytest.mark.parametrize("sizes,hidden,code_act,out_act", PARITY, ids=ident)
def test_parity(Ts, sizes, hidden, code_act, out_act, mode, dt):
    _, got = train(Ts[dt], sizes, mode, hidden, code_act, out_act)
    want_params, want_losses = reference(sizes, dt, hidden, code_act, out_act)
    errs = [rel_err(g, w) for g, w in zip(got[:-1], want_params)] + [loss_err(got[-1], want_losses)]
    print("parity", sizes, dt.__name__, mode, hidden, code_act, out_act, "max error %.2e" % max(errs))
    assert max(errs) <= 5 * RTOL[dt]


# ---- 2. cutting and repeating a chain ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F32, F64], ids=ident)
@pytest.mark.parametrize("mode", [0, 2], ids=["per_sample", "persistent"])
def test_cut_and_repeat(Ts, mode, dt):
    T, sizes, acts = Ts[dt], (13, 7, 4, 13), ("tanh", "identity", "tanh")
    _, whole = train(T, sizes, mode, *acts)
    net, head = train(T, sizes, mode, *acts, idx=IDX[:2])
    _, tail = train(T, sizes, mode, *acts, idx=IDX[2:], net=net)
    assert all_same(tail[:-1], whole[:-1]) and same_bits(np.concatenate([head[-1], tail[-1]]), whole[-1])
    assert all_same(train(T, sizes, mode, *acts)[1], whole)                      # a second identical call
    _, rows = train(T, sizes, mode, *acts, idx=None, n=3)                        # idx null is idx = arange
    assert all_same(rows, train(T, sizes, mode, *acts, idx=(0, 1, 2))[1])
    if mode == 0:                                                                # n_idx = 1 is to_autoencoder_stack_sgd on that row
        ws, X = case(sizes, dt, "tanh")
        W, b = put_net(T, ws)
        l1 = T.autoencoder_sgd(W, b, 2, T.put(X[3:4], batched=True), RATE, "tanh", "squaredError", "tanh", "identity",
                               want_losses=True)
        assert all_same(params(W, b) + [l1.numpy()], train(T, sizes, 0, *acts, idx=(3,))[1])


# ---- 3. route A is the caller's loop of minibatch = 1 --------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F32, F64], ids=ident)
@pytest.mark.parametrize("sizes,out_act", [((12, 8, 5, 8, 12), "softmax"), ((13, 7, 4, 13), "tanh")], ids=ident)
def test_route_a_is_minibatch_one(Ts, sizes, out_act, dt):
    T = Ts[dt]
    ws, X = case(sizes, dt, out_act)
    _, got = train(T, sizes, 0, "tanh", "logistic", out_act)
    W, b = put_net(T, ws)
    losses = T.autoencoder_minibatch_sgd(W, b, PLANS[sizes][0], T.put(X, batched=True), RATE, 1, idx=IDX, out_act=out_act,
                                         loss=AEN.PAIRS[out_act], hidden_act="tanh", code_act="logistic", want_losses=True)
    assert all_same(got, params(W, b) + [losses.numpy()])


# ---- 4. routing ----------------------------------------------------------------------------------------------------------------
def test_routing(Ts):
    from tensor_ops_amd.hipt import HipT
    T = Ts[F32]
    train(T, (12, 8, 5, 8, 12), 2, out_act="softmax", want=(0, 1))               # the softmax pair: route A whatever is asked
    # automatic: only what was scanned -- fp32, two logistic layers, 256 samples or more -- takes the persistent route
    long_idx = tuple(np.arange(256) % N)
    train(T, (5, 3, 5), 1, idx=long_idx, want=(1, 0))
    train(T, (5, 3, 5), 1, want=(0, 1))                                          # a short chain
    train(T, (5, 3, 5), 1, code_act="tanh", idx=long_idx, want=(0, 1))           # a layer that is not logistic
    train(Ts[F64], (5, 3, 5), 1, idx=long_idx, want=(0, 1))                      # fp64
    train(T, (12, 8, 5, 8, 12), 1, idx=long_idx, want=(0, 1))                    # a deeper stack
    HipT.autoencoder_online_groups(0)
    for Tq, sizes in ((T, (2049, 2, 2049)), (Ts[F64], (784, 512, 784))):          # i0 out of range; 200 KiB a workgroup at G = 32
        assert not Tq.autoencoder_online_plan(sizes)["exists"]
        ws, X = problem(list(sizes), 2, Tq.dtype.type, 7, "logistic")
        W, b = put_net(Tq, ws)
        s0 = HipT.autoencoder_online_stats()
        losses = Tq.autoencoder_online_sgd(W, b, 1, Tq.put(X, batched=True), 0.01, idx=[1, 0], want_losses=True)
        assert HipT.autoencoder_online_stats() == (s0[0], s0[1] + 1)
        cur = [(w.astype(F64), bb.astype(F64)) for w, bb in ws]
        want = []
        for q in (1, 0):
            want.append(AEN.run(cur, 1, X[q:q + 1], "logistic", "logistic", "logistic")[2][0])
            cur = AEN.sgd(cur, 1, X[q:q + 1], 0.01, "logistic", "logistic", "logistic")
        errs = [rel_err(g, w) for g, w in zip(params(W, b), [w for w, _ in cur] + [bb for _, bb in cur])]
        assert max(errs + [loss_err(losses.numpy(), np.array(want))]) <= 2 * RTOL[Tq.dtype.type]
    # on route B the launch count does not depend on n_idx; on route A it grows
    def launches(mode, idx):
        train(T, (5, 3, 5), mode, idx=idx)
        l0 = T.stats()["launches"]
        train(T, (5, 3, 5), mode, idx=idx)
        return T.stats()["launches"] - l0
    assert launches(2, IDX[:2]) == launches(2, IDX) and launches(0, IDX[:2]) < launches(0, IDX)


# ---- 5. the contract -------------------------------------------------------------------------------------------------------------
def test_contract(Ts):
    from tensor_ops_amd import capi
    from tensor_ops_amd.hipt import Graph, HipT
    L, T, sizes = capi.lib(), Ts[F32], (13, 7, 4, 13)
    ws, X = case(sizes, F32, "logistic")
    W, b = put_net(T, ws)
    x = T.put(X, batched=True)
    sentinel = lambda k: T.put(np.full(k, 7.5, F32), batched=True)  # noqa: E731
    losses = sentinel(len(IDX))
    start = params(W, b) + [losses.numpy()]
    arr = lambda ts: (capi.c_tensor * len(ts))(*[t.h for t in ts])  # noqa: E731

    def call(Wl=W, k=len(IDX), ii=IDX, out_act=0, loss=0, ll=losses):
        ia = np.ascontiguousarray(ii, np.int64) if ii is not None else None
        return L.to_autoencoder_stack_online_sgd(2, 1, arr(Wl), arr(b), 0, 0, out_act, loss, x.h, k,
                                                 ia.ctypes.data_as(C.POINTER(C.c_int64)) if ia is not None else None, RATE,
                                                 ll if isinstance(ll, (int, type(None))) else ll.h)
    for mode in (0, 2):
        HipT.autoencoder_online_persistent(mode)
        assert call(k=0, ii=None) == ARG                                           # n_idx = 0
        assert call(ii=(2, 0, N, 3, 3)) == SHAPE and call(ii=(2, 0, -1, 3, 3)) == SHAPE   # an index out of range
        assert call(k=N + 1, ii=None, ll=sentinel(N + 1)) == SHAPE                 # idx null with n_idx > N
        assert call(ll=sentinel(len(IDX) + 1)) == SHAPE                            # losses of the wrong batch
        assert call(Wl=W[:2] + [T.put(ws[2][0][:12])]) == SHAPE                    # w[L-1] without i0 rows
        assert call(out_act=2, loss=0) == UNSUPPORTED and call(out_act=3, loss=1) == UNSUPPORTED   # a bad pair
        for base in (x, W[0]):                                                     # losses overlapping X or a parameter
            alias = capi.c_tensor()
            dims, rank = capi.dims_arr(())
            assert L.to_wrap(base.ptr, capi.TO_F32, rank, dims, len(IDX), C.byref(alias)) == 0
            assert call(ll=alias.value) == ARG
            L.to_release(alias)
        with Graph():
            st = call()
        assert st == STATE                                                         # refused while a capture records
        assert all_same(params(W, b) + [losses.numpy()], start) and same_bits(x.numpy(), X)
    assert call() == OK and not np.any(losses.numpy() == F32(7.5)) and not all_same(params(W, b), start[:-1])
    assert L.to_set_autoencoder_online_persistent(3, None) == ARG and L.to_set_autoencoder_online_groups(33, None) == ARG
