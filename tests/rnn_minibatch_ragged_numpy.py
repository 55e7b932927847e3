"""A plain numpy restatement, in float64, of to_rnn_stack_minibatch_sgd_ragged: tests/rnn_minibatch_numpy.py's fold with every
member of a minibatch cut to its own length -- the BPTT of tests/act_numpy.py on X[q][None, :lens[q]], summed over the
minibatch's members, plus the update, each update from what the one before left.  Rows t >= lens[q] are padding: never read,
and the losses there are zero.

A layer is (s, Ws, W, b, state_act) as in act_numpy: s = Ws = state_act = None for a stateless ffLayer.  lens has one entry
per sequence of X, whatever idx names."""
import numpy as np

import act_numpy as AN


def minibatch(layers, X, Y, lens, idx, M, rate_state, rate_params, hidden, out_act):
    """(the layers after the last update, losses [n_idx, T]); losses[j][:lens[idx[j]]] are sequence idx[j]'s under the parameters
    its update started from, the rest +0.0"""
    f64 = lambda v: None if v is None else np.array(v, np.float64)  # noqa: E731
    layers = [tuple(f64(v) for v in lay[:4]) + (lay[4],) for lay in layers]
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    losses = np.zeros((len(idx), X.shape[1]))
    for k in range(0, len(idx), M):
        tot = None
        for j in range(k, min(k + M, len(idx))):
            q, n = idx[j], int(lens[idx[j]])
            g = AN.rnn_bptt(layers, X[q][None, :n], Y[q][None, :n], hidden, out_act)
            losses[j, :n] = g[5][0]
            tot = g[:4] if tot is None else [[None if a is None else a + b for a, b in zip(u, v)] for u, v in zip(tot, g[:4])]
        rates = (rate_state, rate_params, rate_params, rate_params)
        layers = [tuple(None if lay[c] is None else lay[c] - rates[c] * tot[c][l] for c in range(4)) + (lay[4],)
                  for l, lay in enumerate(layers)]
    return layers, losses
