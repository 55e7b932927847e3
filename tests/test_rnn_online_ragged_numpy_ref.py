"""CPU: the numpy restatement of to_rnn_stack_online_sgd_ragged (tests/rnn_online_ragged_numpy.py, what the GPU tests compare
against) is the oracle's `trainNetwork'` (oracle/recurrent.py, Recurrent.hs:326-371) folded over the same sequences in the
same order, each fed as the list of its own lens[q] steps.  Then: with every length T it is the dense restatement exactly,
NaN in every padding row changes no bit, and the lengths matter -- the padded-dense result is another one."""
import numpy as np
import pytest

import rnn_online_numpy as ON
import rnn_online_ragged_numpy as ORN
from oracle import neuralnet as NN, recurrent as R
from test_rnn_numpy_ref import O, close, make, oracle_net, oracle_params, oracle_states
from test_rnn_online_numpy_ref import STACKS

N, T, IDX, LENS = 3, 3, [2, 0, 2], [3, 1, 2]
RATE_STATE, RATE_PARAMS = 0.3, 0.05


def drawn(stack):
    i, spec, out_act, loss, n = stack
    assert n == T
    rng = np.random.default_rng(0x7e500051 + len(spec))
    layers = make(stack)
    X = rng.uniform(-1, 1, (N, T, i))
    Y = rng.uniform(0.1, 0.9, (N, T, spec[-1][0]))
    five = [lay + ("logistic" if lay[1] is not None else None,) for lay in layers]
    return layers, five, X, Y


def fold_oracle(stack, layers, X, Y, idx):
    out_act, loss = stack[2], stack[3]
    net = oracle_net(layers, out_act)
    oloss = {"squaredError": NN.squaredError, "crossEntropy": NN.crossEntropy}[loss]()
    for q in idx:
        net = R.trainNetwork(O, oloss, RATE_STATE, RATE_PARAMS, list(X[q][:LENS[q]]), list(Y[q][:LENS[q]]), net)
    return net


def flat(layers, losses):
    return [v for lay in layers for v in lay[:4] if v is not None] + [losses]


def same_bits(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and np.array_equal(x.view(np.uint64), y.view(np.uint64))
                                    for x, y in zip(a, b))


@pytest.mark.parametrize("stack", STACKS, ids=lambda s: "i%d_L%d_%s" % (s[0], len(s[1]), s[2]))
def test_ragged_online_is_the_oracles_fold(stack):
    out_act, loss = stack[2], stack[3]
    layers, five, X, Y = drawn(stack)
    got, losses = ORN.online(five, X, Y, LENS, IDX, RATE_STATE, RATE_PARAMS, "logistic", out_act)
    net = fold_oracle(stack, layers, X, Y, IDX)
    for l, st in oracle_states(layers, net.state).items():
        close(got[l][0], st)
    for l, d in oracle_params(layers, net.params).items():
        close(got[l][2], d["w"])
        close(got[l][3], d["b"])
        if "ws" in d:
            close(got[l][1], d["ws"])
    assert all(g[0] is None and g[1] is None for g, lay in zip(got, layers) if lay[1] is None)
    # losses[j] is the loss of the leading steps of sequence idx[j] under the parameters step j started from; +0.0 behind them
    assert losses.shape == (len(IDX), T)
    oloss = {"squaredError": NN.squaredError, "crossEntropy": NN.crossEntropy}[loss]()
    q0, q2 = IDX[0], IDX[-1]
    close(losses[0].sum(), R.total_loss(O, oloss, list(X[q0][:LENS[q0]]), list(Y[q0][:LENS[q0]]), oracle_net(layers, out_act)))
    before_last = fold_oracle(stack, layers, X, Y, IDX[:-1])
    close(losses[-1].sum(), R.total_loss(O, oloss, list(X[q2][:LENS[q2]]), list(Y[q2][:LENS[q2]]), before_last))
    for j, q in enumerate(IDX):
        pad = losses[j, LENS[q]:]
        assert np.all(pad == 0.0) and not np.signbit(pad).any()
        assert np.all(losses[j, :LENS[q]] > 0.0)


@pytest.mark.parametrize("stack", STACKS, ids=lambda s: "i%d_L%d_%s" % (s[0], len(s[1]), s[2]))
def test_equal_lengths_padding_and_the_padded_objective(stack):
    out_act = stack[2]
    _, five, X, Y = drawn(stack)
    run = lambda x, y, lens: ORN.online(five, x, y, lens, IDX, RATE_STATE, RATE_PARAMS, "logistic", out_act)  # noqa: E731
    got = flat(*run(X, Y, LENS))
    # every length T: the dense restatement, exactly
    assert same_bits(flat(*run(X, Y, [T] * N)), flat(*ON.online(five, X, Y, IDX, RATE_STATE, RATE_PARAMS, "logistic", out_act)))
    # NaN in every padding row of X and Y: no output bit changes
    Xn, Yn = X.copy(), Y.copy()
    for q in range(N):
        Xn[q, LENS[q]:] = np.nan
        Yn[q, LENS[q]:] = np.nan
    assert np.isnan(Xn).any() and np.isnan(Yn).any()
    assert same_bits(flat(*run(Xn, Yn, LENS)), got)
    # the lengths are not ignored: training on the padded rows ends somewhere else
    padded = flat(*run(X, Y, [T] * N))
    w, wp = got[-3], padded[-3]   # the last layer's W
    assert np.linalg.norm(w - wp) > 1e-6 * np.linalg.norm(w)
    # and the inputs were not modified in place
    assert same_bits(flat(*run(X, Y, LENS)), got)
