"""CPU: the numpy restatement of tests/act_numpy.py (what the GPU tests of the tanh paths of the one-call stack entries
compare against) agrees with the oracle -- `genNet ws (actMap tanh) out`, netGrad, trainNetwork, induceNetwork of
oracle/neuralnet.py; `fullyConnected act`, runNetwork, netGrad, batched_grads of oracle/recurrent.py -- in fp64 at 1e-12,
for both activations, on the smallest stacks those tests use."""
import numpy as np
import pytest

import act_numpy as AN
from oracle import ad, neuralnet as NN, recurrent as R
from oracle.tensor import OTensor
from test_rnn_numpy_ref import oracle_params, oracle_states

O = OTensor(np.float64)
TOL = 1e-12
OACT = {"logistic": NN.actLogistic, "tanh": lambda: NN.actMap(ad.tanh)}
OOUT = {"softmax": NN.actSoftmax, "logistic": NN.actLogistic}
OLOSS = {"softmax": NN.crossEntropy, "logistic": NN.squaredError}

# (sizes, out_act)
FF = [([30, 14, 6], "softmax"), ([30, 14, 6], "logistic"), ([2, 12, 8, 1], "logistic"), ([20, 16, 12, 8, 4], "softmax")]


def close(a, b, tol=TOL):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    assert np.linalg.norm(a - b) <= tol * max(np.linalg.norm(b), 1e-300)


def ff_problem(sizes, B, seed):
    rng = np.random.default_rng(seed)
    ws = [(0.5 * rng.standard_normal((o, i)), 0.5 * rng.standard_normal(o)) for i, o in zip(sizes[:-1], sizes[1:])]
    return ws, rng.uniform(-1, 1, (B, sizes[0])), rng.uniform(0.05, 0.95, (B, sizes[-1]))


# (logistic on two stacks only: act_numpy's logistic branch is the arithmetic of tests/rnn_numpy.py and induce_numpy.py)
FF_CASES = [(s, o, "tanh") for s, o in FF] + [(s, o, "logistic") for s, o in FF[1:3]]


@pytest.mark.parametrize("sizes,out_act,hidden", FF_CASES, ids=lambda v: "-".join(map(str, v)) if isinstance(v, list) else v)
def test_fflayer_stack_matches_oracle(sizes, out_act, hidden):
    B = 3
    ws, X, Y = ff_problem(sizes, B, 0xac7 + len(sizes))
    net = NN.genNet(ws, OACT[hidden], OOUT[out_act])
    loss = OLOSS[out_act]()
    # forward
    _, out = AN.forward(ws, X, hidden, out_act)
    for r in range(B):
        close(out[r], NN.runNetwork(O, net, X[r]))
    # batched gradients, losses, and each row's input cotangent
    g, losses, gx = AN.grads(ws, X, Y, hidden, out_act)
    want = NN.batched_param_grads(O, loss, list(X), list(Y), net)
    for l, (gw, gb) in enumerate(g):
        close(gw, want[2 * l])
        close(gb, want[2 * l + 1])
    close(losses, NN.batched_losses(O, loss, list(X), list(Y), net))
    for r in range(B):
        close(gx[r], NN.netGrad(O, loss, X[r], Y[r], net)[0])
    # the per-sample loop
    cur = net
    order = [2, 0, 1, 2]
    for s in order:
        cur = NN.trainNetwork(O, loss, 0.1, X[s], Y[s], cur)
    for (w, b), pw, pb in zip(AN.online(ws, X, Y, order, 0.1, hidden, out_act), cur.params[0::2], cur.params[1::2]):
        close(w, pw)
        close(b, pb)
    # one sample's sgd step is trainNetwork
    one = NN.trainNetwork(O, loss, 0.3, X[1], Y[1], net)
    for (w, b), pw, pb in zip(AN.sgd(ws, X[1:2], Y[1:2], 0.3, hidden, out_act), one.params[0::2], one.params[1::2]):
        close(w, pw)
        close(b, pb)
    # induceNetwork, three times in a row
    xo, g_last, ls = AN.induce(ws, X[:2], Y[:2], 0.2, 3, hidden, out_act)
    for r in range(2):
        x = X[r]
        for k in range(3):
            close(ls[r, k], NN.batched_losses(O, loss, [x], [Y[r]], net)[0])
            if k == 2:
                close(g_last[r], NN.netGrad(O, loss, x, Y[r], net)[0])
            x = NN.induceNetwork(O, loss, 0.2, Y[r], net, x)
        close(xo[r], x)


# (input, [(n, state_act or None)], hidden_act, out_act, T, B)
RNN = [
    (7, [(12, "tanh"), (9, "logistic"), (5, None)], "tanh", "softmax", 5, 2),
    (7, [(12, "tanh"), (9, "logistic"), (5, None)], "logistic", "softmax", 5, 2),
    (7, [(12, "tanh"), (9, "logistic"), (5, None)], "tanh", "softmax", 1, 1),
    (4, [(6, None), (3, "tanh")], "tanh", "logistic", 3, 2),
]


def rnn_layers(i, spec, rng):
    layers, prev = [], i
    for n, sa in spec:
        W, b = 0.5 * rng.standard_normal((n, prev)), 0.5 * rng.standard_normal(n)
        layers.append((0.5 * rng.standard_normal(n), 0.5 * rng.standard_normal((n, n)), W, b, sa) if sa else (None, None, W, b, None))
        prev = n
    return layers


def oracle_rnn(layers, hidden, out_act):
    def vals(lay):
        s, ws, w, b, sa = lay
        return ((s, ws, w, b), OACT[sa]) if sa else ((w, b), None)
    hid = [(vals(l)[0], OACT[hidden], vals(l)[1]) for l in layers[:-1]]
    return R.genNet(hid, vals(layers[-1]), OOUT[out_act])


@pytest.mark.parametrize("case", RNN, ids=lambda c: "i%d_L%d_%s_T%d" % (c[0], len(c[1]), c[2], c[4]))
def test_rnn_stack_matches_oracle(case):
    i, spec, hidden, out_act, T, B = case
    rng = np.random.default_rng(0x7a4 + T + len(hidden))
    layers = rnn_layers(i, spec, rng)
    net = oracle_rnn(layers, hidden, out_act)
    loss = OLOSS[out_act]()
    X = rng.uniform(-1, 1, (B, T, i))
    Y = rng.uniform(0.1, 0.9, (B, T, spec[-1][0]))
    out, cache = AN.rnn_forward(layers, X, hidden, out_act)
    fin = AN.rnn_final_states(cache)
    for q in range(B):
        cur = net
        for t in range(T):
            yo, cur = R.runNetwork(O, cur, X[q, t])
            close(out[q, t], yo)
        for l, st in oracle_states(layers, cur.state).items():
            close(fin[l][q], st)
    gs, gws, gw, gb, gx, losses = AN.rnn_bptt(layers, X, Y, hidden, out_act)
    xs, ys = [X[:, t] for t in range(T)], [Y[:, t] for t in range(T)]
    want_s, want_p = R.batched_grads(O, loss, xs, ys, net)
    for l, g in oracle_states(layers, want_s).items():
        close(gs[l], g)
    for l, d in oracle_params(layers, want_p).items():
        close(gw[l], d["w"])
        close(gb[l], d["b"])
        if "ws" in d:
            close(gws[l], d["ws"])
    for q in range(B):
        gI, _, _ = R.netGrad(O, loss, list(X[q]), list(Y[q]), net)
        for t in range(T):
            close(gx[q, t], gI[T - 1 - t])   # the reference's inputs' cotangents come in reversed time order
        close(losses[q].sum(), R.total_loss(O, loss, list(X[q]), list(Y[q]), net))
