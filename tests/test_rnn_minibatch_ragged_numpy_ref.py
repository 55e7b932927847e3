"""CPU: the numpy restatement of to_rnn_stack_minibatch_sgd_ragged (tests/rnn_minibatch_ragged_numpy.py, what the GPU tests
compare against) is tests/rnn_online_ragged_numpy.py at M = 1, tests/rnn_minibatch_numpy.py when every length is T, and on one
logistic minibatch the masked batched BPTT of tests/rnn_ragged_numpy.py plus the update."""
import numpy as np

import rnn_minibatch_numpy as MN
import rnn_minibatch_ragged_numpy as MR
import rnn_online_ragged_numpy as OR
import rnn_ragged_numpy as RN
from test_gpu_rnn_tanh import make, rel_err

IDX = [3, 0, 3, 5, 1, 7, 2]
LENS = [5, 1, 3, 4, 2, 2, 5, 3]


def setup(spec):
    rng = np.random.default_rng(0x71 + 5 + 8)
    return make(rng, 7, spec, np.float64), rng.uniform(-1, 1, (8, 5, 7)), rng.uniform(0.1, 0.9, (8, 5, 5))


def worst(got, want):
    (gl, gloss), (wl, wloss) = got, want
    return max([rel_err(g[c], w[c]) for g, w in zip(gl, wl) for c in range(4) if w[c] is not None] + [rel_err(gloss, wloss)])


def test_against_the_three_restatements():
    mixed = [(12, "tanh"), (9, "logistic"), (5, None)]
    layers, X, Y = setup(mixed)
    assert worst(MR.minibatch(layers, X, Y, LENS, IDX, 1, 0.1, 0.02, "tanh", "softmax"),
                 OR.online(layers, X, Y, LENS, IDX, 0.1, 0.02, "tanh", "softmax")) < 1e-10
    assert worst(MR.minibatch(layers, X, Y, [5] * 8, IDX, 3, 0.1, 0.02, "tanh", "softmax"),
                 MN.minibatch(layers, X, Y, IDX, 3, 0.1, 0.02, "tanh", "softmax")) < 1e-10
    # one logistic minibatch: the masked batched BPTT, NaN at the padding, and the update by hand
    layers, X, Y = setup([(12, "logistic"), (5, None)])
    q = IDX[:4]
    Xn, Yn = X.copy(), Y.copy()
    for b in range(8):
        Xn[b, LENS[b]:], Yn[b, LENS[b]:] = np.nan, np.nan
    gs, gws, gw, gb, _, ls = RN.bptt([lay[:4] for lay in layers], Xn[q], Yn[q], [LENS[b] for b in q], "softmax", "crossEntropy")
    want = [tuple(None if v is None else v - r * g[l] for v, r, g in zip(lay[:4], (0.1, 0.02, 0.02, 0.02), (gs, gws, gw, gb)))
            for l, lay in enumerate(layers)]
    assert worst(MR.minibatch(layers, X, Y, LENS, q, 4, 0.1, 0.02, "logistic", "softmax"), (want, ls)) < 1e-10
