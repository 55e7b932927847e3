"""tanh in the recurrent stacks (to_rnn_stack_run / _grad / _sgd): state_act[l] = TO_ACT_TANH per layer, mixed freely with
logistic and stateless layers, and hidden_act = TO_ACT_TANH for the `*~ act` behind every non-final layer.

Checked against the numpy BPTT of tests/act_numpy.py (held to oracle/recurrent.py at 1e-12 by tests/test_act_numpy_ref.py) on
every recurrence route -- per step, automatic, persistent wherever in range (to_set_rnn_persistent 0 / 1 / 2, read back from
to_rnn_stats) -- with hidden_act tanh, and with hidden_act logistic over a tanh state (the layer's output and its state are
then different functions of z).  Tolerances are tests/test_gpu_rnn_stack.py's."""
import numpy as np
import pytest

import act_numpy as AN

pytestmark = pytest.mark.gpu
TOL = {np.float32: 1e-5, np.float64: 1e-11}
CHUNK_TOL = {np.float32: 1e-6, np.float64: 1e-11}   # (test_chunked_run_equals_whole_run: the contractions' row counts differ)
LOSS = {"softmax": "crossEntropy", "logistic": "squaredError"}

# (name, input, [(n, state_act or None)], out_act, T, B, dtypes, persistent under mode 1?)
CASES = [
    ("mixed", 7, [(12, "tanh"), (9, "logistic"), (5, None)], "softmax", 5, 3, [np.float32, np.float64], True),
    ("T1_B1", 7, [(12, "tanh"), (9, "logistic"), (5, None)], "softmax", 1, 1, [np.float32, np.float64], True),
    # one fullyConnected layer of 210 units in fp32: beyond the 201 whose W' the persistent kernel holds in LDS -- per step
    # when automatic, persistent (W' through L2) when forced; it is the output layer, under the logistic head
    ("H210", 6, [(210, "tanh")], "logistic", 3, 2, [np.float32], False),
]
PARAMS = [(c, dt, mode, hidden) for c in CASES for dt in c[6] for mode in (0, 1, 2) for hidden in ("tanh", "logistic")]


@pytest.fixture(scope="module")
def Ts():
    from tensor_ops_amd.hipt import HipT
    return {np.float32: HipT(0, np.float32), np.float64: HipT(0, np.float64)}


def rel_err(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    den = np.linalg.norm(want.ravel())
    return np.linalg.norm((got - want).ravel()) / (den if den > 0 else 1.0)


def make(rng, i, spec, dt):
    layers, prev = [], i
    for n, sa in spec:
        W, b = rng.standard_normal((n, prev)) / np.sqrt(prev), 0.5 * rng.standard_normal(n)
        s, ws = (0.5 * rng.standard_normal(n), rng.standard_normal((n, n)) / np.sqrt(n)) if sa else (None, None)
        layers.append(tuple(None if v is None else np.asarray(v, dt) for v in (s, ws, W, b)) + (sa,))
        prev = n
    return layers


def dev(T, layers):
    return [tuple(None if v is None else T.put(v) for v in lay[:4]) + (lay[4] if lay[4] else False,) for lay in layers]


def ident(v):
    if isinstance(v, tuple):
        return v[0]
    return getattr(v, "__name__", str(v))


@pytest.mark.parametrize("case,dt,mode,hidden", PARAMS, ids=ident)
def test_run_grad_sgd(Ts, case, dt, mode, hidden):
    name, i, spec, out_act, n, B, _, auto_persistent = case
    T, tol = Ts[dt], TOL[dt]
    rng = np.random.default_rng(0x52 + n + B)
    layers = make(rng, i, spec, dt)
    X = rng.uniform(-1, 1, (B, n, i)).astype(dt)
    Y = rng.uniform(0.1, 0.9, (B, n, spec[-1][0])).astype(dt)
    stateful = [l for l, lay in enumerate(layers) if lay[4]]
    prev = T.rnn_persistent(mode)
    try:
        dl = dev(T, layers)
        x, y = T.put(X, batched=True), T.put(Y, batched=True)
        # run: every step's output and the final states; the route the stats name
        p0, q0 = T.rnn_stats()
        out, fin = T.rnn_stack_run(dl, x, out_act, want_states=True, hidden_act=hidden)
        p1, q1 = T.rnn_stats()
        persistent = mode == 2 or (mode == 1 and auto_persistent)
        assert (p1 - p0, q1 - q0) == ((1, 0) if persistent else (0, 1))
        want_out, cache = AN.rnn_forward(layers, X, hidden, out_act)
        want_fin = AN.rnn_final_states(cache)
        errs = [rel_err(out.numpy(), want_out)] + [rel_err(fin[l].numpy(), want_fin[l]) for l in stateful]
        print("run", errs)
        assert max(errs) < tol
        if n > 1:   # fed in two chunks, the second from the first one's final states
            a, fa = T.rnn_stack_run(dl, T.put(X[:, :2], batched=True), out_act, want_states=True, hidden_act=hidden)
            dl2 = [((fa[l],) + lay[1:]) if lay[0] is not None else lay for l, lay in enumerate(dl)]
            c, fc = T.rnn_stack_run(dl2, T.put(X[:, 2:], batched=True), out_act, want_states=True, hidden_act=hidden)
            assert rel_err(np.concatenate([a.numpy(), c.numpy()], axis=1), out.numpy()) < CHUNK_TOL[dt]
            for l in stateful:
                assert rel_err(fc[l].numpy(), fin[l].numpy()) < CHUNK_TOL[dt]
        # grad (k: tests/test_gpu_rnn_stack.py allows 5 tol on sums over a batch of sequences)
        k = 5 if B > 1 else 1
        gS, gWS, gW, gB, gx, losses = T.rnn_stack_grad(dl, x, y, out_act, LOSS[out_act], want_gx=True, want_losses=True,
                                                       hidden_act=hidden)
        ws_, wws, ww, wb, wgx, wl = AN.rnn_bptt(layers, X, Y, hidden, out_act)
        errs = [rel_err(gW[l].numpy(), ww[l]) for l in range(len(layers))] + [rel_err(gB[l].numpy(), wb[l]) for l in range(len(layers))]
        errs += [rel_err(gS[l].numpy(), ws_[l]) for l in stateful] + [rel_err(gWS[l].numpy(), wws[l]) for l in stateful]
        errs += [rel_err(gx.numpy(), wgx), rel_err(losses.numpy(), wl)]
        print("grad", errs)
        assert max(errs) < k * tol
        assert all(gS[l] is None and gWS[l] is None for l in range(len(layers)) if l not in stateful)
        # sgd: trainNetwork' with rate_state != rate_params
        rs, rp = 0.3, 0.05
        T.rnn_stack_sgd(dl, x, y, rs, rp, out_act, LOSS[out_act], hidden_act=hidden)
        errs = []
        for l, lay in enumerate(layers):
            errs += [rel_err(dl[l][2].numpy(), lay[2].astype(np.float64) - rp * ww[l]),
                     rel_err(dl[l][3].numpy(), lay[3].astype(np.float64) - rp * wb[l])]
            if lay[4]:
                errs += [rel_err(dl[l][0].numpy(), lay[0].astype(np.float64) - rs * ws_[l]),
                         rel_err(dl[l][1].numpy(), lay[1].astype(np.float64) - rp * wws[l])]
        print("sgd", errs)
        assert max(errs) < k * tol
    finally:
        T.rnn_persistent(prev)


def test_layer_description(Ts):
    """the state activation of the Python layer tuples: absent / True is logistic, "tanh" is tanh, and a value that does not
    fit the layer's kind is refused before anything is called"""
    T = Ts[np.float32]
    rng = np.random.default_rng(3)
    layers = make(rng, 4, [(6, "logistic"), (3, None)], np.float32)
    X = rng.uniform(-1, 1, (2, 3, 4)).astype(np.float32)
    x = T.put(X, batched=True)
    four = [tuple(None if v is None else T.put(v) for v in lay[:4]) for lay in layers]
    a, _ = T.rnn_stack_run(four, x)
    b, _ = T.rnn_stack_run([four[0] + (True,), four[1] + (False,)], x)
    c, _ = T.rnn_stack_run([four[0] + ("logistic",), four[1]], x)
    assert np.array_equal(a.numpy(), b.numpy()) and np.array_equal(a.numpy(), c.numpy())
    d, _ = T.rnn_stack_run([four[0] + ("tanh",), four[1]], x)
    assert not np.array_equal(a.numpy(), d.numpy())
    with pytest.raises(ValueError):
        T.rnn_stack_run([four[0] + (False,), four[1]], x)
    with pytest.raises(ValueError):
        T.rnn_stack_run([four[0], four[1] + ("tanh",)], x)
