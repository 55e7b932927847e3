"""Recurrent stacks in one call (to_rnn_stack_run / _grad / _sgd, csrc/rnn_seq.hip): `runNetwork` threaded over time,
BPTT summed over a hidden batch of sequences and `trainNetwork'` of Recurrent.hs.

Small stacks are checked against the oracle (oracle/recurrent.py) and the host mirror's generic BPTT; stacks at size
against the fp64 numpy BPTT of tests/rnn_numpy.py (itself checked against the oracle in test_rnn_numpy_ref.py), on both
recurrence routes -- the persistent kernel and the per-step launches -- which must agree.  Then: launches independent of T,
determinism, independence of a sequence from its batch, chunked runs, and the call's contract."""
import ctypes as C

import numpy as np
import pytest

import rnn_numpy as RN
from oracle import neuralnet as NN, recurrent as R
from oracle.tensor import OTensor
from test_rnn_numpy_ref import oracle_net, oracle_params, oracle_states

pytestmark = pytest.mark.gpu
O = OTensor(np.float64)
TOL = {np.float32: 1e-5, np.float64: 1e-11}


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


def rel_err(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    den = np.linalg.norm(want.ravel())
    return np.linalg.norm((got - want).ravel()) / (den if den > 0 else 1.0)


def make(rng, i, spec, dt, scale=0.5):
    layers, prev = [], i
    for n, st in spec:
        W, b = scale * rng.standard_normal((n, prev)), scale * rng.standard_normal(n)
        s, ws = (scale * rng.standard_normal(n), scale * rng.standard_normal((n, n))) if st else (None, None)
        layers.append(tuple(None if v is None else np.asarray(v, dt) for v in (s, ws, W, b)))
        prev = n
    return layers


def dev(T, layers):
    return [tuple(None if v is None else T.put(v) for v in lay) for lay in layers]


def data(rng, B, T, i, o, dt):
    X = rng.uniform(-1, 1, (B, T, i)).astype(dt)
    Y = rng.uniform(0.1, 0.9, (B, T, o)).astype(dt)
    return X, Y


def put_seq(T, A, batched):
    return T.put(A, batched=True) if batched else T.put(A[0])


# (i, [(n, stateful)] input to output, out_act, loss, T): tests/test_gpu_recurrent.py's CASES (a logistic hidden layer
# there is `actLogistic` or `actMapLogistic`: the same map), a stateful output layer under softmax, odd widths, T = 1
CASES = [
    (2, [(3, True)], "logistic", "squaredError", 4),
    (3, [(4, True), (5, False), (2, True)], "softmax", "crossEntropy", 3),
    (6, [(8, True), (4, False)], "softmax", "crossEntropy", 5),
    (4, [(4, True)], "logistic", "squaredError", 1),
    (5, [(6, False), (7, True)], "softmax", "crossEntropy", 4),
    (9, [(37, True), (300, True), (11, False)], "softmax", "crossEntropy", 3),
]


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("B", [0, 7], ids=["unbatched", "B7"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "i%d_L%d_T%d" % (c[0], len(c[1]), c[4]))
def test_oracle_parity(Ts, dt, B, case):
    T = Ts[dt]
    tol = TOL[dt]
    i, spec, out_act, loss, n = case
    rng = np.random.default_rng(hash((i, n, B)) & 0xffff)
    layers = make(rng, i, spec, dt)
    net = oracle_net([tuple(None if v is None else v.astype(np.float64) for v in lay) for lay in layers], out_act)
    oloss = {"squaredError": NN.squaredError, "crossEntropy": NN.crossEntropy}[loss]()
    X, Y = data(rng, max(B, 1), n, i, spec[-1][0], dt)
    dl = dev(T, layers)
    x, y = put_seq(T, X, B > 0), put_seq(T, Y, B > 0)
    # run: every step's output and the final states, sequence by sequence against runNetwork threaded over time
    out, fin = T.rnn_stack_run(dl, x, out_act, want_states=True)
    out = out.numpy().reshape(max(B, 1), n, -1)
    for q in range(max(B, 1)):
        cur = net
        for t in range(n):
            yo, cur = R.runNetwork(O, cur, X[q, t].astype(np.float64))
            assert rel_err(out[q, t], yo) < tol
        for l, st in oracle_states(layers, cur.state).items():
            assert rel_err(fin[l].numpy().reshape(max(B, 1), -1)[q], st) < tol
    # grad: batched_grads (sums over the sequences), netGrad per sequence for the inputs' cotangents
    gS, gWS, gW, gB, gx, losses = T.rnn_stack_grad(dl, x, y, out_act, loss, want_gx=True, want_losses=True)
    xs, ys = [X[:, t].astype(np.float64) for t in range(n)], [Y[:, t].astype(np.float64) for t in range(n)]
    want_s, want_p = R.batched_grads(O, oloss, xs, ys, net)
    k = 5 if B else 1
    for l, g in oracle_states(layers, want_s).items():
        assert gS[l].batch == 0 and rel_err(gS[l].numpy(), g) < k * tol
    for l, d in oracle_params(layers, want_p).items():
        assert rel_err(gW[l].numpy(), d["w"]) < k * tol and rel_err(gB[l].numpy(), d["b"]) < k * tol
        if "ws" in d:
            assert rel_err(gWS[l].numpy(), d["ws"]) < k * tol
    q = 3 if B else 0
    gI, _, _ = R.netGrad(O, oloss, [x_[q] for x_ in xs], [y_[q] for y_ in ys], net)
    gxn = gx.numpy().reshape(max(B, 1), n, i)
    for t in range(n):
        assert rel_err(gxn[q, t], gI[n - 1 - t]) < k * tol   # the reference's order is reversed in time
    tot = sum(R.total_loss(O, oloss, [x_[p] for x_ in xs], [y_[p] for y_ in ys], net) for p in range(max(B, 1)))
    assert abs(float(losses.numpy().sum()) - tot) <= k * tol * abs(tot)
    # sgd: trainNetwork' with rate_state != rate_params (B sequences: the summed gradient)
    rs, rp = 0.3, 0.05
    T.rnn_stack_sgd(dl, x, y, rs, rp, out_act, loss)
    if B == 0:
        new = R.trainNetwork(O, oloss, rs, rp, [v[0] for v in xs], [v[0] for v in ys], net)
        want_s, want_p = oracle_states(layers, new.state), oracle_params(layers, new.params)
    else:
        want_s = {l: layers[l][0].astype(np.float64) - rs * g for l, g in oracle_states(layers, want_s).items()}
        want_p = {l: {kk: {"ws": layers[l][1], "w": layers[l][2], "b": layers[l][3]}[kk].astype(np.float64) - rp * v
                      for kk, v in d.items()} for l, d in oracle_params(layers, want_p).items()}
    for l, st in want_s.items():
        assert rel_err(dl[l][0].numpy(), st) < k * tol
    for l, d in want_p.items():
        for kk, v in d.items():
            assert rel_err(dl[l][{"ws": 1, "w": 2, "b": 3}[kk]].numpy(), v) < k * tol


def test_host_mirror_parity(Ts):
    """the host mirror's generic BPTT (rnn_netGrad in a memo scope) on the same network"""
    from tensor_ops_amd import tops
    tops.hlib()
    T = Ts[np.float32]
    tops.set_elem_dtype(np.float32)
    rng = np.random.default_rng(5)
    i, n, B = 3, 4, 7
    layers = make(rng, i, [(4, True), (5, False), (2, True)], np.float32)
    dl = dev(T, layers)
    net_h = tops.rnn_genNet([(dl[0], "actLogistic", "actLogistic"), ((dl[1][2], dl[1][3]), "actLogistic", None)],
                            (dl[2], "actLogistic"), "actSoftmax")
    X, Y = data(rng, B, n, i, 2, np.float32)
    xs = [T.put(X[:, t], batched=True) for t in range(n)]
    ys = [T.put(Y[:, t], batched=True) for t in range(n)]
    with T.memo():
        hI, hS, hP = tops.rnn_netGrad(net_h, "crossEntropy", xs, ys)
    gS, gWS, gW, gB, gx, _ = T.rnn_stack_grad(dl, T.put(X, batched=True), T.put(Y, batched=True), "softmax",
                                              "crossEntropy", want_gx=True)
    for l, g in oracle_states(layers, hS).items():
        assert rel_err(gS[l].numpy(), g.numpy()) < 5e-5
    for l, d in oracle_params(layers, hP).items():
        assert rel_err(gW[l].numpy(), d["w"].numpy()) < 5e-5 and rel_err(gB[l].numpy(), d["b"].numpy()) < 5e-5
        if "ws" in d:
            assert rel_err(gWS[l].numpy(), d["ws"].numpy()) < 5e-5
    gxn = gx.numpy()
    for t in range(n):
        assert rel_err(gxn[:, t], hI[n - 1 - t].numpy()) < 5e-5


SIZES = [  # (dtype, i, spec, T, B)
    (np.float32, 128, [(512, True), (256, True), (10, False)], 128, 256),
    (np.float64, 32, [(512, True), (10, False)], 64, 64),
]


@pytest.mark.parametrize("size", SIZES, ids=["f32_512_256_T128_B256", "f64_512_T64_B64"])
def test_at_size_both_routes(Ts, size):
    from tensor_ops_amd.hipt import HipT
    dt, i, spec, n, B = size
    T = Ts[dt]
    rng = np.random.default_rng(77)
    layers = make(rng, i, spec, dt, scale=0.1)
    X, Y = data(rng, B, n, i, spec[-1][0], dt)
    Y = (Y / Y.sum(axis=-1, keepdims=True)).astype(dt)
    gs, gws, gw, gb, gx, losses = RN.bptt(layers, X, Y, "softmax", "crossEntropy")
    want_out, _ = RN.forward(layers, X, "softmax")
    tol = 1e-4 if dt == np.float32 else 1e-10
    dl = dev(T, layers)
    x, y = T.put(X, batched=True), T.put(Y, batched=True)
    got = {}
    for mode in (2, 0):
        HipT.rnn_persistent(mode)
        p0, s0 = HipT.rnn_stats()
        out, _ = T.rnn_stack_run(dl, x, "softmax")
        gS, gWS, gW, gB, gX, L = T.rnn_stack_grad(dl, x, y, "softmax", "crossEntropy", want_gx=True, want_losses=True)
        p1, s1 = HipT.rnn_stats()
        assert (p1 - p0, s1 - s0) == ((2, 0) if mode == 2 else (0, 2))
        assert rel_err(out.numpy(), want_out) < tol
        for l in range(len(layers)):
            assert rel_err(gW[l].numpy(), gw[l]) < tol and rel_err(gB[l].numpy(), gb[l]) < tol
            if gs[l] is not None:
                assert rel_err(gS[l].numpy(), gs[l]) < tol and rel_err(gWS[l].numpy(), gws[l]) < tol
        assert rel_err(gX.numpy(), gx) < tol and rel_err(L.numpy(), losses) < tol
        got[mode] = [g.numpy() for g in gW + gB] + [gX.numpy()]
    for a, b in zip(got[2], got[0]):   # the two routes agree
        assert rel_err(a, b) < tol


def test_above_persistent_range_runs_per_step(Ts):
    from tensor_ops_amd.hipt import HipT
    T = Ts[np.float32]
    rng = np.random.default_rng(8)
    H = 1100   # > RNN_SEQ_MAX_H
    layers = make(rng, 16, [(H, True), (5, False)], np.float32, scale=0.05)
    X, Y = data(rng, 2, 3, 16, 5, np.float32)
    Y = (Y / Y.sum(axis=-1, keepdims=True)).astype(np.float32)
    HipT.rnn_persistent(2)
    p0, s0 = HipT.rnn_stats()
    gS, gWS, gW, gB, _, _ = T.rnn_stack_grad(dev(T, layers), T.put(X, batched=True), T.put(Y, batched=True))
    p1, s1 = HipT.rnn_stats()
    assert (p1 - p0, s1 - s0) == (0, 1)
    gs, gws, gw, gb, _, _ = RN.bptt(layers, X, Y, "softmax", "crossEntropy")
    assert rel_err(gWS[0].numpy(), gws[0]) < 1e-4 and rel_err(gS[0].numpy(), gs[0]) < 1e-4
    assert rel_err(gW[0].numpy(), gw[0]) < 1e-4 and rel_err(gW[1].numpy(), gw[1]) < 1e-4


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["f32", "f64"])
def test_launches_do_not_depend_on_T(Ts, dt):
    from tensor_ops_amd.hipt import HipT
    T = Ts[dt]
    HipT.rnn_persistent(2)
    rng = np.random.default_rng(3)
    layers = make(rng, 8, [(64, True), (32, True), (10, False)], dt)
    dl = dev(T, layers)

    def launches(n):
        X, Y = data(rng, 16, n, 8, 10, dt)
        x, y = T.put(X, batched=True), T.put(Y, batched=True)
        T.rnn_stack_grad(dl, x, y, want_gx=True)
        l0 = T.stats()["launches"]
        T.rnn_stack_grad(dl, x, y, want_gx=True)
        return T.stats()["launches"] - l0
    a, b = launches(8), launches(128)
    assert a == b, (a, b)
    HipT.rnn_persistent(0)
    assert launches(8) < launches(16)   # the per-step route grows with T


def test_deterministic_and_independent_of_the_batch(Ts):
    from tensor_ops_amd.hipt import HipT
    T = Ts[np.float32]
    HipT.rnn_persistent(2)
    rng = np.random.default_rng(11)
    layers = make(rng, 6, [(48, True), (20, True), (7, False)], np.float32)
    dl = dev(T, layers)
    X, Y = data(rng, 9, 12, 6, 7, np.float32)
    x, y = T.put(X, batched=True), T.put(Y, batched=True)
    g1 = [t.numpy() for t in sum(T.rnn_stack_grad(dl, x, y, want_gx=True)[2:4], [])]
    g2 = [t.numpy() for t in sum(T.rnn_stack_grad(dl, x, y, want_gx=True)[2:4], [])]
    for a, b in zip(g1, g2):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    out = T.rnn_stack_run(dl, x, "softmax")[0].numpy()
    alone = T.rnn_stack_run(dl, T.put(X[4]), "softmax")[0].numpy()
    perm = np.roll(np.arange(9), 3)
    moved = T.rnn_stack_run(dl, T.put(X[perm], batched=True), "softmax")[0].numpy()
    assert rel_err(alone, out[4]) < 1e-6
    assert rel_err(moved[np.argsort(perm)], out) < 1e-6


def test_chunked_run_equals_whole_run(Ts):
    """run over T = run over T1, then over T2 from the first call's s_out (within 1e-6: the row counts of the contractions
    differ between the calls, so the bits need not)"""
    T = Ts[np.float32]
    rng = np.random.default_rng(12)
    layers = make(rng, 5, [(24, True), (6, False), (9, True)], np.float32)
    dl = dev(T, layers)
    X, _ = data(rng, 4, 10, 5, 9, np.float32)
    whole, fin = T.rnn_stack_run(dl, T.put(X, batched=True), "logistic", want_states=True)
    a, fa = T.rnn_stack_run(dl, T.put(X[:, :6], batched=True), "logistic", want_states=True)
    dl2 = [(fa[l], lay[1], lay[2], lay[3]) if lay[0] is not None else lay for l, lay in enumerate(dl)]
    b, fb = T.rnn_stack_run(dl2, T.put(X[:, 6:], batched=True), "logistic", want_states=True)
    assert rel_err(np.concatenate([a.numpy(), b.numpy()], axis=1), whole.numpy()) < 1e-6
    for l in (0, 2):
        assert rel_err(fb[l].numpy(), fin[l].numpy()) < 1e-6


def test_contract(Ts):
    from tensor_ops_amd import capi
    from tensor_ops_amd.hipt import Graph, HipT
    L = capi.lib()
    T, T64 = Ts[np.float32], Ts[np.float64]
    rng = np.random.default_rng(13)
    layers = make(rng, 4, [(6, True), (3, False)], np.float32)
    dl = dev(T, layers)
    X, Y = data(rng, 5, 4, 4, 3, np.float32)
    x, y = T.put(X, batched=True), T.put(Y, batched=True)
    before = [[None if v is None else v.numpy() for v in lay] for lay in dl]

    def sgd(layers_=dl, xx=x, yy=y, out_act=2, loss=1, hidden=0, sact=(0, -1)):
        n = len(layers_)
        arr = lambda k: (capi.c_tensor * n)(*[(lay[k].h if lay[k] is not None else None) for lay in layers_])  # noqa
        return L.to_rnn_stack_sgd(n, (C.c_int * n)(*sact), arr(0), arr(1), arr(2), arr(3), hidden, out_act, loss, xx.h,
                                  yy.h, 0.1, 0.1, None)
    assert sgd(xx=T.put(X[:, :, :3], batched=True)) == 2                        # X does not fit W_1
    assert sgd(yy=T.put(Y[:, :, :2], batched=True)) == 2                        # Y not n_L wide
    assert sgd(yy=T.put(Y[:4], batched=True)) == 2                              # Y of another batch
    assert sgd(yy=T.put(Y[:, :3], batched=True)) == 2                           # Y of another length
    assert sgd(yy=T64.put(Y.astype(np.float64), batched=True)) == 1             # dtype mix
    assert sgd(out_act=2, loss=0) == 5 and sgd(out_act=0, loss=1) == 5           # pairs outside the contract
    assert sgd(hidden=2) == 5 and sgd(sact=(2, -1)) == 5                         # activations outside the contract
    assert sgd(sact=(-1, -1)) == 1                                               # a stateless layer given a state
    s_b = T.put(np.tile(layers[0][0], (5, 1)), batched=True)                      # batched initial state in grad / sgd
    assert sgd(layers_=[(s_b,) + dl[0][1:], dl[1]]) == 2
    with Graph():
        st = sgd()
    assert st == 4                                                               # refused while a capture records
    for lay, want in zip(dl, before):
        for v, w in zip(lay, want):
            if v is not None:
                assert np.array_equal(v.numpy().view(np.uint8), w.view(np.uint8))   # nothing was written
    assert sgd() == 0
    assert not np.array_equal(dl[0][1].numpy(), before[0][1])
    assert HipT.rnn_persistent(1) == 1 and L.to_set_rnn_persistent(3, None) == 1
