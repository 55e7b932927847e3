"""The wide recurrent route (csrc/rnn_wide.hip, to_set_rnn_wide): W' split by columns over the workgroups of a group, one
launch per layer and direction.  Against the fp64 numpy BPTT of tests/rnn_numpy.py (tests/act_numpy.py for tanh states), at
the smallest shapes at which the kernel can go wrong; then the routes' agreement, determinism, independence of a row from
its batch, and the switches' contract."""
import numpy as np
import pytest

import act_numpy as AN
import rnn_numpy as RN
from test_gpu_rnn_stack import data, dev, rel_err

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
TOL = {F32: 1e-4, F64: 1e-10}   # test_at_size_both_routes' tolerances for wide layers, weights of scale 0.1


@pytest.fixture(scope="module")
def Ts():
    from tensor_ops_amd.hipt import HipT
    return {F32: HipT(0, F32), F64: HipT(0, F64)}


@pytest.fixture(autouse=True)
def switches():
    from tensor_ops_amd.hipt import HipT
    wide, groups, pers = HipT.rnn_wide(2), HipT.rnn_wide_groups(0), HipT.rnn_persistent(1)
    yield wide
    HipT.rnn_wide(wide), HipT.rnn_wide_groups(groups), HipT.rnn_persistent(pers)


def make(rng, i, spec, dt):
    """[(s, W', W, b, state_act)] for spec [(n, state_act or None)], weights of scale 0.1"""
    layers, prev = [], i
    for n, sact in spec:
        W, b = 0.1 * rng.standard_normal((n, prev)), 0.1 * rng.standard_normal(n)
        s, ws = (0.1 * rng.standard_normal(n), 0.1 * rng.standard_normal((n, n))) if sact else (None, None)
        layers.append(tuple(None if v is None else np.asarray(v, dt) for v in (s, ws, W, b)) + (sact or True,))
        prev = n
    return layers


def reference(layers, X, Y, out_act):
    """(out, final states, (gs, gws, gw, gb, gx, losses)) in fp64"""
    if any(lay[4] == "tanh" for lay in layers):
        out, cache = AN.rnn_forward(layers, X, "logistic", out_act)
        return out, AN.rnn_final_states(cache), AN.rnn_bptt(layers, X, Y, "logistic", out_act)
    plain = [lay[:4] for lay in layers]
    out, cache = RN.forward(plain, X, out_act)
    return out, RN.final_states(cache), RN.bptt(plain, X, Y, out_act, "crossEntropy" if out_act == "softmax" else "squaredError")


ONE = lambda H, sact="logistic": (6, [(H, sact), (5, None)], "softmax")   # noqa: E731  i = 6 -> H (stateful) -> 5
# (dtype, (i, spec, out_act), B, T, min_groups)
CASES = [
    (F32, ONE(202), 1, 1, 0),            # the first width in range, one row, T = 1: no exchange at all
    (F32, ONE(203), 1, 4, 0),            # odd H, a short last slab, both parity slots rewritten
    (F32, ONE(203), 3, 3, 32),           # C = 7, G lowered to 29, three groups
    (F32, ONE(257), 5, 3, 0),
    (F32, ONE(257), 16, 3, 0),           # FMA form with two rows a group, all eight groups
    (F32, ONE(257, "tanh"), 17, 3, 0),   # three rows a group, the last group with two; tanh state
    (F32, ONE(257), 40, 3, 0),           # MFMA form, rows padded 5 -> 16, C = 129: nine column blocks over eight waves
    (F32, ONE(257, "tanh"), 128, 2, 0),  # MFMA form, full 16 rows, K slices summed across waves
    (F64, ONE(143), 2, 3, 0),            # two words a value
    (F64, ONE(260), 9, 2, 0),            # fp64 FMA form, R = 2, uneven groups
    (F64, ONE(260), 72, 2, 0),           # fp64 MFMA form, R = 9
    (F32, (8, [(210, "tanh"), (230, "logistic"), (4, None)], "logistic"), 2, 3, 0),   # wide layers back to back
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s_H%s_B%d_T%d_g%d" % (
    "f64" if c[0] is F64 else "f32", "_".join("%d%s" % (n, (a or "")[:1]) for n, a in c[1][1][:-1]), c[2], c[3], c[4]))
def test_parity(Ts, case):
    from tensor_ops_amd.hipt import HipT
    dt, (i, spec, out_act), B, n, min_groups = case
    T, tol = Ts[dt], TOL[dt]
    loss = "crossEntropy" if out_act == "softmax" else "squaredError"
    rng = np.random.default_rng(5)
    layers = make(rng, i, spec, dt)
    X, Y = data(rng, B, n, i, spec[-1][0], dt)
    if out_act == "softmax":
        Y = (Y / Y.sum(axis=-1, keepdims=True)).astype(dt)
    want_out, want_fin, (gs, gws, gw, gb, gx, losses) = reference(layers, X, Y, out_act)
    HipT.rnn_wide_groups(min_groups)
    nw = sum(1 for _, a in spec if a)
    x, y, dl = T.put(X, batched=True), T.put(Y, batched=True), dev(T, [lay[:4] for lay in layers])
    dl = [d + (lay[4],) for d, lay in zip(dl, layers)]
    launches = lambda: HipT.rnn_wide_stats()[0]   # noqa: E731

    l0 = launches()
    out, fin = T.rnn_stack_run(dl, x, out_act, want_states=True)
    assert launches() - l0 == nw
    assert rel_err(out.numpy(), want_out) < tol
    for l in range(nw):
        assert rel_err(fin[l].numpy(), want_fin[l]) < tol

    l0 = launches()
    gS, gWS, gW, gB, gX, L = T.rnn_stack_grad(dl, x, y, out_act, loss, want_gx=True, want_losses=True)
    assert launches() - l0 == 2 * nw
    for l in range(len(layers)):
        assert rel_err(gW[l].numpy(), gw[l]) < tol and rel_err(gB[l].numpy(), gb[l]) < tol
        if gs[l] is not None:
            assert rel_err(gS[l].numpy(), gs[l]) < tol and rel_err(gWS[l].numpy(), gws[l]) < tol
    assert rel_err(gX.numpy(), gx) < tol and rel_err(L.numpy(), losses) < tol

    l0 = launches()
    T.rnn_stack_sgd(dl, x, y, 0.05, 0.1, out_act, loss)   # in place: dl is not used again
    assert launches() - l0 == 2 * nw
    for l, lay in enumerate(layers):
        for k, (g, rate) in enumerate(((gs[l], 0.05), (gws[l], 0.1), (gw[l], 0.1), (gb[l], 0.1))):
            if g is not None:
                assert rel_err(dl[l][k].numpy(), np.asarray(lay[k], F64) - rate * g) < tol
    assert HipT.rnn_wide_stats()[1] == 0


def grad_of(T, layers, X, Y):
    dl = dev(T, [lay[:4] for lay in layers])
    res = T.rnn_stack_grad(dl, T.put(X, batched=True), T.put(Y, batched=True), want_gx=True, want_losses=True)
    return [t.numpy() for t in res[0][:1] + res[1][:1] + res[2] + res[3] + [res[4], res[5]]]


def test_routes_agree(Ts):
    from tensor_ops_amd.hipt import HipT
    rng = np.random.default_rng(6)
    layers = make(rng, 6, [(257, "logistic"), (5, None)], F32)
    X, Y = data(rng, 5, 4, 6, 5, F32)
    wide = grad_of(Ts[F32], layers, X, Y)
    HipT.rnn_wide(0), HipT.rnn_persistent(0)
    l0 = HipT.rnn_wide_stats()[0]
    step = grad_of(Ts[F32], layers, X, Y)
    assert HipT.rnn_wide_stats()[0] == l0
    for a, b in zip(wide, step):
        assert rel_err(a, b) < TOL[F32]


@pytest.mark.parametrize("B", [5, 40], ids=["B5_fma", "B40_mfma"])
def test_deterministic_and_independent_of_the_other_rows(Ts, B):
    rng = np.random.default_rng(7)
    layers = make(rng, 6, [(257, "logistic"), (5, None)], F32)
    X, Y = data(rng, B, 4, 6, 5, F32)
    bits = lambda a: a.view(np.uint8)   # noqa: E731
    g1, g2 = grad_of(Ts[F32], layers, X, Y), grad_of(Ts[F32], layers, X, Y)
    for a, b in zip(g1, g2):
        assert np.array_equal(bits(a), bits(b))
    X2, Y2 = data(rng, B, 4, 6, 5, F32)   # row 0 kept, every other row replaced: the same B, so the same plan
    X2[0], Y2[0] = X[0], Y[0]
    g3 = grad_of(Ts[F32], layers, X2, Y2)
    assert np.array_equal(bits(g1[-2][0]), bits(g3[-2][0])) and np.array_equal(bits(g1[-1][0]), bits(g3[-1][0]))
    assert not np.array_equal(bits(g1[-2][1]), bits(g3[-2][1]))


def test_contract(Ts, switches):
    from tensor_ops_amd import capi
    from tensor_ops_amd.hipt import HipT
    L = capi.lib()
    assert L.to_set_rnn_wide(3, None) == 1 and L.to_set_rnn_wide_groups(33, None) == 1   # TO_ERR_ARG
    assert HipT.rnn_wide(1) == 2 and HipT.rnn_wide(2) == 1                              # the previous value comes back
    assert not HipT.rnn_wide_plan(201, 1)["exists"] and HipT.rnn_wide_plan(202, 1)["exists"]
    assert not HipT.rnn_wide_plan(142, 1, "f64")["exists"] and HipT.rnn_wide_plan(143, 1, "f64")["exists"]
    assert not HipT.rnn_wide_plan(1025, 1)["exists"] and not HipT.rnn_wide_plan(257, 129)["exists"]   # RNN_SEQ_MAX_H + 1; B
    assert not HipT.rnn_wide_plan(1024, 1, "f64")["exists"]                              # no G <= 32 fits the slab
    HipT.rnn_wide_groups(32)
    p = HipT.rnn_wide_plan(203, 3)
    assert (p["exists"], p["G"], p["C"]) == (True, 29, 7)
    HipT.rnn_wide_groups(0)
    for dt, H, B in ((F32, 202, 1), (F32, 257, 40), (F32, 512, 128), (F32, 1024, 24), (F64, 260, 72)):
        p = HipT.rnn_wide_plan(H, B, "f64" if dt is F64 else "f32")
        assert p["exists"] and p["lds_bytes"] <= 160 * 1024 and p["mfma"] == (p["R"] > 4) and p["groups"] * p["R"] >= B
    # the default (what `switches` found and put aside) is off, and leaves a wide layer on today's routes
    assert switches == 0
    HipT.rnn_wide(switches)
    rng = np.random.default_rng(8)
    layers = make(rng, 6, [(257, "logistic"), (5, None)], F32)
    X, Y = data(rng, 2, 3, 6, 5, F32)
    l0, s0 = HipT.rnn_wide_stats()[0], HipT.rnn_stats()
    grad_of(Ts[F32], layers, X, Y)
    s1 = HipT.rnn_stats()
    assert HipT.rnn_wide_stats()[0] == l0 and (s1[0] - s0[0], s1[1] - s0[1]) == (0, 1)
