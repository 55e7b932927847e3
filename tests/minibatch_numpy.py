"""Minibatch SGD over a data set restated in numpy: `act_numpy.sgd` chained over the gathered rows, one step a minibatch,
the gradient SUMMED over the minibatch (what to_fflayer_stack_minibatch_sgd computes).  tests/test_minibatch_numpy_ref.py
ties its two ends to act_numpy: minibatches of one row are `act_numpy.online`, one minibatch of every row is one
`act_numpy.sgd`."""
import numpy as np

import act_numpy as AN


def batches(n_idx, M):
    """the (start, stop) of every minibatch of n_idx samples in order; the last may be short"""
    return [(s, min(s + M, n_idx)) for s in range(0, n_idx, M)]


def minibatch_sgd(ws, X, Y, order, M, rate, hidden, out_act, dt=np.float64):
    """(parameters after the last step, losses [len(order)]: the loss of row order[j] under the parameters its step started
    from).  Y None: the target of a row is the row itself."""
    order = np.asarray(order, np.int64)
    X = np.asarray(X)
    Y = X if Y is None else np.asarray(Y)
    ws = [(np.asarray(w, dt), np.asarray(b, dt)) for w, b in ws]
    losses = np.zeros(len(order), dt)
    for s, e in batches(len(order), M):
        rows = order[s:e]
        _, losses[s:e], _ = AN.grads(ws, X[rows], Y[rows], hidden, out_act, dt)
        ws = AN.sgd(ws, X[rows], Y[rows], rate, hidden, out_act, dt)
    return ws, losses
