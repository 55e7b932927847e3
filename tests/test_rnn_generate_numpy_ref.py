"""CPU: the numpy restatement of closed-loop generation (tests/rnn_generate_numpy.py, what tests/test_gpu_rnn_generate.py
states the feed rule with) agrees with the oracle -- `runNetwork` of oracle/recurrent.py threaded over the fed inputs -- in
fp64 at 1e-12; the feed rules do what the public header says on hand-made rows; and the stacks the GPU cases use visit at
least 3 distinct symbols in every row over G = 12 (a closed loop that collapses onto one symbol tests no wiring)."""
import numpy as np
import pytest

import rnn_generate_numpy as GN
from oracle import ad, neuralnet as NN, recurrent as R
from oracle.tensor import OTensor
from test_rnn_numpy_ref import oracle_states

O = OTensor(np.float64)
OACT = {"logistic": NN.actLogistic, "tanh": lambda: NN.actMap(ad.tanh)}
OOUT = {"softmax": NN.actSoftmax, "logistic": NN.actLogistic}

# (name, i = n_L, [(n, state_act or None)] input to output, out_act, hidden_act, the seed of GN.shift_stack): the seeds are the
# ones for which every row of the numpy closed loop shows at least 3 distinct symbols (test_input_diversity)
CASES = [
    ("L1", 5, [(5, "tanh")], "softmax", "logistic", 0),
    ("L2", 5, [(7, "logistic"), (5, None)], "softmax", "logistic", 1),
    ("L2w", 6, [(37, "tanh"), (6, "logistic")], "softmax", "logistic", 9),
    ("L3", 5, [(8, None), (9, "logistic"), (5, "tanh")], "softmax", "logistic", 3),
    ("sq", 4, [(6, "tanh"), (4, None)], "logistic", "tanh", 2),
]
ONE_HOT = [c for c in CASES if c[3] == "softmax"]


def oracle_net(layers, hidden, out_act):
    """test_rnn_numpy_ref.oracle_net with each layer's own state activation and the stack's hidden activation"""
    def vals(lay):
        s, ws, w, b, sa = lay
        return ((s, ws, w, b), OACT[sa]) if sa else ((w, b), None)
    hid = [(vals(l)[0], OACT[hidden], vals(l)[1]) for l in layers[:-1]]
    return R.genNet(hid, vals(layers[-1]), OOUT[out_act])


def oracle_open_loop(layers, hidden, out_act, xs):
    """runNetwork threaded over the rows of xs [T, i] from the stack's own (unbatched) states: (outputs [T, n_L], final
    states by layer)"""
    cur, outs = oracle_net(layers, hidden, out_act), []
    for x in xs:
        y, cur = R.runNetwork(O, cur, np.asarray(x, np.float64))
        outs.append(y)
    return np.stack(outs), oracle_states(layers, cur.state)


def prime_data(seed, B, Tp, i, G, dt=np.float64):
    """X [B, Tp, i]: one-hot rows of random symbols; U [B, G] uniform in [0, 1)"""
    rng = np.random.default_rng(1000 + seed)
    X = GN.one_hot(rng.integers(0, i, B * Tp), i, dt).reshape(B, Tp, i)
    return X, rng.uniform(0, 1, (B, G)).astype(dt)


def close(a, b, tol=1e-12):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    assert np.linalg.norm(a - b) <= tol * max(np.linalg.norm(b), 1e-300)


# (the logistic head is fed back as it is)
CASE_MODES = [(c, m) for c in CASES for m in (("output", "argmax", "sample") if c[3] == "softmax" else ("output",))]


@pytest.mark.parametrize("case,mode", CASE_MODES, ids=lambda v: v[0] if isinstance(v, tuple) else v)
def test_step_matches_oracle(case, mode):
    name, i, spec, out_act, hidden, seed = case
    layers = GN.shift_stack(seed, i, spec)
    B, Tp, G = 3, 2, 5
    X, U = prime_data(seed, B, Tp, i, G)
    out, sym, prime, states, fed = GN.generate(layers, X, G, mode, U, hidden, out_act)
    assert out.shape == (B, G, i) and prime.shape == (B, Tp, i) and fed.shape == (B, G, i)
    for q in range(B):
        want, fin = oracle_open_loop(layers, hidden, out_act, np.concatenate([X[q], fed[q]]))
        close(prime[q], want[:Tp])
        close(out[q], want[Tp:])
        for l, st in fin.items():
            close(states[l][q], st)
    # the closed loop: every fed row is the rule applied to the row before it
    prev = np.concatenate([prime[:, -1:], out[:, :-1]], axis=1)
    for k in range(G):
        x, c = GN.feed(prev[:, k], mode, U[:, k])
        assert np.array_equal(x, fed[:, k]) and (c is None or np.array_equal(c, sym[:, k]))


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["f32", "f64"])
def test_feed_rules(dt):
    p = np.array([[0.1, 0.4, 0.4, 0.1], [0.25, 0.25, 0.25, 0.25], [0.0, 0.0, 1.0, 0.0]], dt)
    x, c = GN.feed(p, "argmax")
    assert c.tolist() == [1, 0, 2] and np.array_equal(x, GN.one_hot(np.array([1, 0, 2]), 4, dt)) and x.dtype == dt   # ties: the earliest index
    x, c = GN.feed(p, "output")
    assert c is None and np.array_equal(x, p)
    # inverse CDF: u = 0 takes the first symbol with mass, u just below a boundary the symbol before it, u = 1 is capped
    assert GN.feed(p, "sample", np.array([0, 0, 0], dt))[1].tolist() == [0, 0, 2]
    assert GN.feed(p, "sample", np.array([1, 1, 1], dt))[1].tolist() == [3, 3, 3]
    assert GN.feed(p, "sample", np.array([0.3, 0.3, 0.3], dt))[1].tolist() == [1, 1, 2]
    assert GN.feed(p, "sample", np.array([0.95, 0.5, 0.999], dt))[1].tolist() == [3, 2, 2]
    # the statement of the rule, element by element in the row's dtype
    rng = np.random.default_rng(4)
    rows = rng.uniform(0, 1, (64, 11)).astype(dt)
    rows /= rows.sum(axis=1, keepdims=True)
    u = rng.uniform(0, 1, 64).astype(dt)
    got = GN.feed(rows, "sample", u)[1]
    for r in range(64):
        acc, cum = dt(0), []
        for v in rows[r]:
            acc = dt(acc + v)
            cum.append(acc)
        thr = dt(u[r] * cum[-1])
        assert got[r] == min(sum(1 for v in cum if v <= thr), 10)


@pytest.mark.parametrize("case", ONE_HOT, ids=lambda c: c[0])
@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("mode", ["argmax", "sample"])
def test_input_diversity(case, dt, mode):
    """the condition the GPU cases rest on: at least 3 distinct symbols in every row over G = 12, at both prime lengths"""
    name, i, spec, out_act, hidden, seed = case
    layers = GN.shift_stack(seed, i, spec, dt)
    for Tp in (1, 3):
        X, U = prime_data(seed, 7, Tp, i, 12, dt)
        sym = GN.generate(layers, X, 12, mode, U, hidden, out_act, dt)[1]
        assert min(len(set(r)) for r in sym.tolist()) >= 3, sym
