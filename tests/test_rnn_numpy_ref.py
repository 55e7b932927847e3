"""CPU: the numpy BPTT of tests/rnn_numpy.py (what the at-size GPU tests of to_rnn_stack_* compare against) agrees with
the oracle's restatement of Recurrent.hs -- runNetwork threaded over time, netGrad per sequence (its inputs' cotangents in
the reference's reversed order), batched_grads, trainNetwork' -- on small stacks of both layer kinds."""
import numpy as np
import pytest

import rnn_numpy as RN
from oracle import neuralnet as NN, recurrent as R
from oracle.tensor import OTensor

O = OTensor(np.float64)
RNG = np.random.default_rng(0x7e500017)

# (i, [(n, stateful)] input to output, out_act, loss, T)
STACKS = [
    (2, [(3, True)], "logistic", "squaredError", 4),
    (3, [(4, True), (5, False), (2, True)], "softmax", "crossEntropy", 3),
    (6, [(8, True), (4, False)], "softmax", "crossEntropy", 5),
    (4, [(4, True)], "logistic", "squaredError", 1),
]


def make(stack):
    i, spec, out_act, loss, T = stack
    layers, prev = [], i
    for n, st in spec:
        W, b = 0.5 * RNG.standard_normal((n, prev)), 0.5 * RNG.standard_normal(n)
        layers.append((0.5 * RNG.standard_normal(n), 0.5 * RNG.standard_normal((n, n)), W, b) if st else (None, None, W, b))
        prev = n
    return layers


def oracle_net(layers, out_act):
    def vals(lay):
        s, ws, w, b = lay
        return ((s, ws, w, b), NN.actLogistic) if ws is not None else ((w, b), None)
    hidden = [(vals(l)[0], NN.actLogistic, vals(l)[1]) for l in layers[:-1]]
    oact = NN.actSoftmax if out_act == "softmax" else NN.actLogistic
    return R.genNet(hidden, vals(layers[-1]), oact)


def oracle_states(layers, vec):
    """the oracle lists states later layers first (`~*~`: ss2 ++ ss1)"""
    idx = [l for l, lay in enumerate(layers) if lay[1] is not None]
    return dict(zip(reversed(idx), vec))


def oracle_params(layers, vec):
    out, k = {}, 0
    for l, lay in enumerate(layers):
        if lay[1] is not None:
            out[l] = {"ws": vec[k], "w": vec[k + 1], "b": vec[k + 2]}
            k += 3
        else:
            out[l] = {"w": vec[k], "b": vec[k + 1]}
            k += 2
    return out


def close(a, b, tol=1e-10):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    assert np.linalg.norm(a - b) <= tol * max(np.linalg.norm(b), 1e-300)


@pytest.mark.parametrize("stack", STACKS, ids=lambda s: "i%d_L%d_T%d" % (s[0], len(s[1]), s[4]))
def test_numpy_bptt_matches_oracle(stack):
    i, spec, out_act, loss, T = stack
    layers = make(stack)
    net = oracle_net(layers, out_act)
    oloss = {"squaredError": NN.squaredError, "crossEntropy": NN.crossEntropy}[loss]()
    xs = RNG.uniform(-1, 1, (T, i))
    ys = RNG.uniform(0.1, 0.9, (T, spec[-1][0]))
    # runNetwork threaded over the steps: outputs and final states
    out, cache = RN.forward(layers, xs[None], out_act)
    cur = net
    for t in range(T):
        yo, cur = R.runNetwork(O, cur, xs[t])
        close(out[0, t], yo)
    fin = RN.final_states(cache)
    for l, st in oracle_states(layers, cur.state).items():
        close(fin[l][0], st)
    # netGrad of one sequence
    gs, gws, gw, gb, gx, losses = RN.bptt(layers, xs[None], ys[None], out_act, loss)
    gI, gS, gP = R.netGrad(O, oloss, list(xs), list(ys), net)
    for l, g in oracle_states(layers, gS).items():
        close(gs[l], g)
    for l, d in oracle_params(layers, gP).items():
        close(gw[l], d["w"])
        close(gb[l], d["b"])
        if "ws" in d:
            close(gws[l], d["ws"])
    for t in range(T):
        close(gx[0, t], gI[T - 1 - t])   # the reference's inputs' cotangents come in reversed time order
    close(losses.sum(), R.total_loss(O, oloss, list(xs), list(ys), net))
    # batched_grads: sums over B sequences
    B = 3
    Xb = RNG.uniform(-1, 1, (B, T, i))
    Yb = RNG.uniform(0.1, 0.9, (B, T, spec[-1][0]))
    gs, gws, gw, gb, _, _ = RN.bptt(layers, Xb, Yb, out_act, loss)
    want_s, want_p = R.batched_grads(O, oloss, [Xb[:, t] for t in range(T)], [Yb[:, t] for t in range(T)], net)
    for l, g in oracle_states(layers, want_s).items():
        close(gs[l], g)
    for l, d in oracle_params(layers, want_p).items():
        close(gw[l], d["w"])
        close(gb[l], d["b"])
        if "ws" in d:
            close(gws[l], d["ws"])
