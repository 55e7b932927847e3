"""A plain numpy restatement of `induceNetwork` (FeedForward.hs:150-164) iterated on the rows of a batch: gradient descent
on the INPUT of a genNet stack (logistic hidden layers) with the parameters fixed -- what to_fflayer_stack_induce computes.
tests/test_induce_numpy_ref.py checks it against oracle.neuralnet.induceNetwork; tests/test_gpu_induce.py uses it where the
oracle would be too slow.  `dtype` is the precision every step is carried in (float64: the reference; float32: what a
device route in fp32 may at best reproduce).

ws = [(W_1, b_1), ...] input to output; X [B, i0]; Y [B, n_L] (or [n_L]: one target for every row)."""
import numpy as np


def sig(x):
    return 1.0 / (1.0 + np.exp(-x))


def grad_x(ws, X, Y, out_act, loss, dtype=np.float64):
    """(dL/dx [B, i0], losses [B]) at X, in `dtype`"""
    ws = [(np.asarray(w, dtype), np.asarray(b, dtype)) for w, b in ws]
    a = np.asarray(X, dtype)
    Y = np.broadcast_to(np.asarray(Y, dtype), (a.shape[0], ws[-1][0].shape[0]))
    acts = []
    for l, (w, b) in enumerate(ws):
        z = a @ w.T + b
        if l + 1 < len(ws):
            a = sig(z)
            acts.append(a)
    if out_act == "softmax":
        assert loss == "crossEntropy"
        e = np.exp(z - z.max(axis=-1, keepdims=True))
        p = e / e.sum(axis=-1, keepdims=True)
        dz = p * Y.sum(axis=-1, keepdims=True) - Y
        losses = -(Y * np.log(p)).sum(axis=-1)
    else:
        assert out_act == "logistic" and loss == "squaredError"
        s = sig(z)
        dz = -2 * (Y - s) * s * (1 - s)
        losses = ((Y - s) ** 2).sum(axis=-1)
    for l in range(len(ws) - 1, 0, -1):
        h = acts[l - 1]
        dz = (dz @ ws[l][0]) * h * (1 - h)
    return (dz @ ws[0][0]).astype(dtype), losses.astype(dtype)


def induce(ws, X, Y, rate, iters, out_act="softmax", loss="crossEntropy", dtype=np.float64):
    """(x_iters [B, i0], the gradient of the last iteration [B, i0] or None, losses [B, iters]: the loss BEFORE each step)"""
    x = np.array(X, dtype)
    g, trace = None, np.empty((x.shape[0], iters), dtype)
    for k in range(iters):
        g, trace[:, k] = grad_x(ws, x, Y, out_act, loss, dtype)
        x = (x - dtype(rate) * g).astype(dtype)
    return x, g, trace
