"""A plain numpy restatement of BPTT for the recurrent stacks of to_rnn_stack_* (fullyConnected layers of Recurrent.hs:91-119
and stateless ffLayers), in time order and float64, batched over independent sequences.  tests/test_rnn_numpy_ref.py checks
it against oracle/recurrent.py on small shapes; tests/test_gpu_rnn_stack.py uses it where the oracle would be too slow.

A layer is (s, Ws, W, b): s [n] or [B, n] and Ws = W' [n, n] for a fullyConnected layer, None and None for an ffLayer.
X is [B, T, i]; every hidden layer's output activation is logistic, the last layer's `out_act`."""
import numpy as np


def sig(x):
    return 1.0 / (1.0 + np.exp(-x))


def softmax(z):
    e = np.exp(z - z.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


def forward(layers, X, out_act):
    """(out [B, T, n_L], per-layer cache (input, z, states [B, T+1, n] or None, output))"""
    X = np.asarray(X, np.float64)
    B, T, _ = X.shape
    a, cache = X, []
    for l, (s, Ws, W, b) in enumerate(layers):
        last = l == len(layers) - 1
        Z = a @ np.asarray(W, np.float64).T + np.asarray(b, np.float64)
        S = None
        if Ws is not None:
            Ws = np.asarray(Ws, np.float64)
            S = np.empty((B, T + 1, W.shape[0]))
            S[:, 0] = np.asarray(s, np.float64)
            for t in range(T):
                Z[:, t] = Z[:, t] + S[:, t] @ Ws.T
                S[:, t + 1] = sig(Z[:, t])
        out = (softmax(Z) if out_act == "softmax" else sig(Z)) if last else sig(Z)
        cache.append((a, Z, S, out))
        a = out
    return a, cache


def final_states(cache):
    return [c[2][:, -1] if c[2] is not None else None for c in cache]


def bptt(layers, X, Y, out_act, loss):
    """objective sum_b sum_t loss(out_bt, Y_bt): (gs, gWs, gW, gb per layer -- states unbatched --, gx [B, T, i],
    losses [B, T])"""
    Y = np.asarray(Y, np.float64)
    _, cache = forward(layers, X, out_act)
    Z = cache[-1][1]
    if out_act == "softmax":
        assert loss == "crossEntropy"
        p = softmax(Z)
        dZ = p * Y.sum(axis=-1, keepdims=True) - Y
        losses = -(Y * np.log(p)).sum(axis=-1)
    else:
        assert loss == "squaredError"
        sz = sig(Z)
        dZ = -2.0 * (Y - sz) * sz * (1.0 - sz)
        losses = ((Y - sz) ** 2).sum(axis=-1)
    n = len(layers)
    gs, gws, gw, gb = [None] * n, [None] * n, [None] * n, [None] * n
    gx = None
    for l in range(n - 1, -1, -1):
        s, Ws, W, b = layers[l]
        a_in, _, S, _ = cache[l]
        dZ = dZ.copy()
        if Ws is not None:
            Ws = np.asarray(Ws, np.float64)
            h = S[:, 1:]
            for t in range(dZ.shape[1] - 2, -1, -1):
                dZ[:, t] += (dZ[:, t + 1] @ Ws) * h[:, t] * (1.0 - h[:, t])
            gws[l] = np.einsum("btj,btk->jk", dZ, S[:, :-1])
            gs[l] = (dZ[:, 0] @ Ws).sum(axis=0)
        gw[l] = np.einsum("btj,btk->jk", dZ, a_in)
        gb[l] = dZ.sum(axis=(0, 1))
        da = dZ @ np.asarray(W, np.float64)
        if l > 0:
            h = cache[l - 1][3]
            dZ = da * h * (1.0 - h)
        else:
            gx = da
    return gs, gws, gw, gb, gx, losses
