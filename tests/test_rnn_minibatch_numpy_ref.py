"""CPU: the numpy restatement of to_rnn_stack_minibatch_sgd (tests/rnn_minibatch_numpy.py, what the GPU tests compare against)
is tests/rnn_online_numpy.py at M = 1 (held to the oracle's trainNetwork by tests/test_rnn_online_numpy_ref.py), and at M = N
one update is act_numpy's batched BPTT plus the update written out by hand."""
import numpy as np

import act_numpy as AN
import rnn_minibatch_numpy as MN
import rnn_online_numpy as ON
from test_gpu_rnn_tanh import make, rel_err

SPEC = [(12, "tanh"), (9, "logistic"), (5, None)]   # "mixed" of tests/test_gpu_rnn_minibatch.py
IDX = [3, 0, 3, 5, 1, 7, 2]


def setup():
    rng = np.random.default_rng(0x71 + 5 + 8 + len("mixed"))
    layers = make(rng, 7, SPEC, np.float64)
    return layers, rng.uniform(-1, 1, (8, 5, 7)), rng.uniform(0.1, 0.9, (8, 5, 5))


def test_minibatch_of_one_is_online():
    layers, X, Y = setup()
    got, gl = MN.minibatch(layers, X, Y, IDX, 1, 0.1, 0.02, "tanh", "softmax")
    want, wl = ON.online(layers, X, Y, IDX, 0.1, 0.02, "tanh", "softmax")
    errs = [rel_err(g[c], w[c]) for g, w in zip(got, want) for c in range(4) if w[c] is not None] + [rel_err(gl, wl)]
    assert max(errs) < 1e-12


def test_one_update_of_the_whole_set_is_bptt_and_the_update():
    layers, X, Y = setup()
    got, gl = MN.minibatch(layers, X, Y, np.arange(8), 8, 0.1, 0.02, "logistic", "softmax")
    gs, gws, gw, gb, _, ls = AN.rnn_bptt(layers, X, Y, "logistic", "softmax")
    errs = [rel_err(gl, ls)]
    for l, (s, Ws, W, b, _) in enumerate(layers):
        errs += [rel_err(got[l][2], W - 0.02 * gw[l]), rel_err(got[l][3], b - 0.02 * gb[l])]
        if Ws is not None:
            errs += [rel_err(got[l][0], s - 0.1 * gs[l]), rel_err(got[l][1], Ws - 0.02 * gws[l])]
    assert max(errs) < 1e-12
    # a short last minibatch is trained on, and the order of the updates matters
    a, _ = MN.minibatch(layers, X, Y, IDX, 3, 0.1, 0.02, "tanh", "softmax")
    b6, _ = MN.minibatch(layers, X, Y, IDX[:6], 3, 0.1, 0.02, "tanh", "softmax")
    c, _ = MN.minibatch(layers, X, Y, IDX[3:] + IDX[:3], 3, 0.1, 0.02, "tanh", "softmax")
    assert rel_err(a[0][2], b6[0][2]) > 1e-6 and rel_err(a[0][2], c[0][2]) > 1e-6
