"""A plain numpy restatement, in float64, of to_rnn_stack_minibatch_sgd: tests/rnn_online_numpy.py with a batch -- the BPTT of
tests/act_numpy.py on X[idx[k M : (k + 1) M]] plus the update, each update from what the one before left.

A layer is (s, Ws, W, b, state_act) as in act_numpy: s = Ws = state_act = None for a stateless ffLayer."""
import numpy as np

import act_numpy as AN


def minibatch(layers, X, Y, idx, M, rate_state, rate_params, hidden, out_act):
    """(the layers after the last update, losses [n_idx, T]); losses[j] are sequence idx[j]'s under the parameters its update
    started from"""
    f64 = lambda v: None if v is None else np.array(v, np.float64)  # noqa: E731
    layers = [tuple(f64(v) for v in lay[:4]) + (lay[4],) for lay in layers]
    X, Y, idx = np.asarray(X, np.float64), np.asarray(Y, np.float64), np.asarray(idx, np.int64)
    losses = np.zeros((len(idx), X.shape[1]))
    for k in range(0, len(idx), M):
        q = idx[k:k + M]
        gs, gws, gw, gb, _, losses[k:k + M] = AN.rnn_bptt(layers, X[q], Y[q], hidden, out_act)
        layers = [(None, None, W - rate_params * gw[l], b - rate_params * gb[l], sact) if Ws is None else
                  (s - rate_state * gs[l], Ws - rate_params * gws[l], W - rate_params * gw[l], b - rate_params * gb[l], sact)
                  for l, (s, Ws, W, b, sact) in enumerate(layers)]
    return layers, losses
