"""CPU: the numpy restatement of to_rnn_stack_online_sgd (tests/rnn_online_numpy.py, what the GPU tests compare against) is
the oracle's `trainNetwork'` (oracle/recurrent.py, Recurrent.hs:326-371) folded over the same sequences in the same order --
each step from the parameters and the learned initial states the step before returned -- and the order matters."""
import numpy as np
import pytest

import rnn_online_numpy as ON
from oracle import neuralnet as NN, recurrent as R
from test_rnn_numpy_ref import O, close, make, oracle_net, oracle_params, oracle_states

# (i, [(n, stateful)] input to output, out_act, loss, T): a stateful -> stateless stack, and one stateful layer under the
# logistic head
STACKS = [
    (3, [(4, True), (2, False)], "softmax", "crossEntropy", 3),
    (3, [(4, True)], "logistic", "squaredError", 3),
]
N, IDX = 3, [2, 0, 2]
RATE_STATE, RATE_PARAMS = 0.3, 0.05


def fold_oracle(stack, layers, X, Y, idx):
    i, spec, out_act, loss, T = stack
    net = oracle_net(layers, out_act)
    oloss = {"squaredError": NN.squaredError, "crossEntropy": NN.crossEntropy}[loss]()
    for q in idx:
        net = R.trainNetwork(O, oloss, RATE_STATE, RATE_PARAMS, list(X[q]), list(Y[q]), net)
    return net


@pytest.mark.parametrize("stack", STACKS, ids=lambda s: "i%d_L%d_%s" % (s[0], len(s[1]), s[2]))
def test_online_is_the_oracles_fold(stack):
    i, spec, out_act, loss, T = stack
    rng = np.random.default_rng(0x7e500041 + len(spec))
    layers = make(stack)
    X = rng.uniform(-1, 1, (N, T, i))
    Y = rng.uniform(0.1, 0.9, (N, T, spec[-1][0]))
    five = [lay + ("logistic" if lay[1] is not None else None,) for lay in layers]
    got, losses = ON.online(five, X, Y, IDX, RATE_STATE, RATE_PARAMS, "logistic", out_act)
    net = fold_oracle(stack, layers, X, Y, IDX)
    for l, st in oracle_states(layers, net.state).items():
        close(got[l][0], st)
    for l, d in oracle_params(layers, net.params).items():
        close(got[l][2], d["w"])
        close(got[l][3], d["b"])
        if "ws" in d:
            close(got[l][1], d["ws"])
    assert all(g[0] is None and g[1] is None for g, lay in zip(got, layers) if lay[1] is None)
    # losses[j] is the loss of sequence idx[j] under the parameters step j started from
    assert losses.shape == (len(IDX), T)
    oloss = {"squaredError": NN.squaredError, "crossEntropy": NN.crossEntropy}[loss]()
    close(losses[0].sum(), R.total_loss(O, oloss, list(X[IDX[0]]), list(Y[IDX[0]]), oracle_net(layers, out_act)))
    before_last = fold_oracle(stack, layers, X, Y, IDX[:-1])
    close(losses[-1].sum(), R.total_loss(O, oloss, list(X[IDX[-1]]), list(Y[IDX[-1]]), before_last))
    # the order matters: a permuted idx ends somewhere else
    other, _ = ON.online(five, X, Y, [0, 2, 2], RATE_STATE, RATE_PARAMS, "logistic", out_act)
    assert np.linalg.norm(other[0][2] - got[0][2]) > 1e-6 * np.linalg.norm(got[0][2])
    # and the inputs were not modified in place
    again, _ = ON.online(five, X, Y, IDX, RATE_STATE, RATE_PARAMS, "logistic", out_act)
    assert all(np.array_equal(a[2], g[2]) for a, g in zip(again, got))
