"""CPU: the numpy restatement of iterated `induceNetwork` (tests/induce_numpy.py, what the GPU tests of
to_fflayer_stack_induce compare against at size) agrees with oracle.neuralnet.induceNetwork applied step by step, and its
gradient with netGrad's input cotangent, in fp64 to 1e-12 -- both heads, one-hot and soft, unnormalised targets."""
import numpy as np
import pytest

import induce_numpy as IN
from oracle import neuralnet as NN
from oracle.tensor import OTensor

O = OTensor(np.float64)
STACKS = [[6, 4], [5, 9, 3], [7, 12, 8, 10], [3, 6, 5, 7, 40]]
HEADS = [("softmax", "crossEntropy"), ("logistic", "squaredError")]


def oracle_net(ws, out_act):
    return NN.genNet([(w, b) for w, b in ws], NN.actLogistic, NN.actSoftmax if out_act == "softmax" else NN.actLogistic)


def oracle_loss(loss):
    return {"squaredError": NN.squaredError, "crossEntropy": NN.crossEntropy}[loss]()


@pytest.mark.parametrize("soft", [False, True], ids=["onehot", "soft"])
@pytest.mark.parametrize("head", HEADS, ids=lambda h: h[0])
@pytest.mark.parametrize("sizes", STACKS, ids=lambda s: "-".join(map(str, s)))
def test_numpy_induce_matches_the_oracle(sizes, head, soft):
    out_act, loss = head
    rng = np.random.default_rng(len(sizes) * 100 + sizes[-1])
    ws = [(0.5 * rng.standard_normal((o, i)), 0.5 * rng.standard_normal(o)) for i, o in zip(sizes[:-1], sizes[1:])]
    B, iters, rate = 5, 6, 0.3
    X = rng.uniform(-1, 1, (B, sizes[0]))
    if soft:
        Y = rng.uniform(0.1, 1, (B, sizes[-1]))
    else:
        Y = np.zeros((B, sizes[-1]))
        Y[np.arange(B), rng.integers(0, sizes[-1], B)] = 1
    net, ol = oracle_net(ws, out_act), oracle_loss(loss)
    got, gx, trace = IN.induce(ws, X, Y, rate, iters, out_act, loss)
    for r in range(B):
        x = X[r]
        for k in range(iters):
            g = np.asarray(NN.netGrad(O, ol, x, Y[r], net)[0], np.float64)
            # the restatement's gradient at the oracle's x_k, its loss there, and one step
            gk, lk = IN.grad_x(ws, x[None], Y[r][None], out_act, loss)
            assert np.abs(gk[0] - g).max() <= 1e-12
            assert abs(lk[0] - trace[r, k]) <= 1e-12 * max(1.0, abs(lk[0]))
            x = np.asarray(NN.induceNetwork(O, ol, rate, Y[r], net, x), np.float64)
        assert np.abs(gx[r] - g).max() <= 1e-12           # gx is the gradient of the LAST iteration
        assert np.abs(got[r] - x).max() <= 1e-12
    assert np.abs(got - X).max() > 1e-3                   # the steps moved x


def test_losses_are_the_oracles_and_an_unbatched_target_is_tiled():
    sizes = [7, 12, 8, 10]
    rng = np.random.default_rng(5)
    ws = [(0.5 * rng.standard_normal((o, i)), 0.5 * rng.standard_normal(o)) for i, o in zip(sizes[:-1], sizes[1:])]
    X = rng.uniform(-1, 1, (3, 7))
    y = rng.uniform(0.1, 1, 10)
    for out_act, loss in HEADS:
        net, ol = oracle_net(ws, out_act), oracle_loss(loss)
        a, ga, ta = IN.induce(ws, X, y, 0.3, 4, out_act, loss)
        b, gb, tb = IN.induce(ws, X, np.tile(y, (3, 1)), 0.3, 4, out_act, loss)
        assert np.array_equal(a, b) and np.array_equal(ga, gb) and np.array_equal(ta, tb)
        want = NN.batched_losses(O, ol, list(X), [y] * 3, net)
        assert np.abs(ta[:, 0] - want).max() <= 1e-12     # losses[:, 0] is the loss at x itself
    x0, g0, t0 = IN.induce(ws, X, y, 0.3, 0)
    assert np.array_equal(x0, X) and g0 is None and t0.shape == (3, 0)
