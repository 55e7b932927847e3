"""A plain numpy restatement, in float64, of to_rnn_stack_online_sgd_ragged: tests/rnn_online_numpy.py's fold with every
sequence cut to its own length -- the BPTT of tests/act_numpy.py on X[q][None, :lens[q]] plus the update, each step starting
from the parameters and the learned initial states the step before left.  Rows t >= lens[q] are padding: they are never
read, and the losses there are zero.  tests/test_rnn_online_ragged_numpy_ref.py holds it to oracle/recurrent.py's
trainNetwork at 1e-10; the GPU tests of tests/test_gpu_rnn_online_ragged.py compare against it.

A layer is (s, Ws, W, b, state_act) as in act_numpy: s = Ws = state_act = None for a stateless ffLayer.  lens has one
entry per sequence of X, whatever idx names."""
import numpy as np

import act_numpy as AN


def online(layers, X, Y, lens, idx, rate_state, rate_params, hidden, out_act):
    """(the layers after the last step, losses [n_idx, T]); losses[j][:lens[idx[j]]] are sequence idx[j]'s under the
    parameters step j started from, the rest +0.0"""
    f64 = lambda v: None if v is None else np.array(v, np.float64)  # noqa: E731
    layers = [tuple(f64(v) for v in lay[:4]) + (lay[4],) for lay in layers]
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    losses = np.zeros((len(idx), X.shape[1]))
    for j, q in enumerate(idx):
        n = int(lens[q])
        gs, gws, gw, gb, _, ls = AN.rnn_bptt(layers, X[q][None, :n], Y[q][None, :n], hidden, out_act)
        losses[j, :n] = ls[0]
        nxt = []
        for l, (s, Ws, W, b, sact) in enumerate(layers):
            if Ws is None:
                nxt.append((None, None, W - rate_params * gw[l], b - rate_params * gb[l], sact))
            else:
                nxt.append((s - rate_state * gs[l], Ws - rate_params * gws[l], W - rate_params * gw[l],
                            b - rate_params * gb[l], sact))
        layers = nxt
    return layers, losses
