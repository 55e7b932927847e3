"""A plain numpy restatement, in float64 unless asked otherwise and parameterised by the hidden / state activation ("logistic" or "tanh"), of what
the one-call stack entries compute: forward, batched parameter gradients, the sgd step, the per-sample online loop,
`induceNetwork` iterated, and BPTT of recurrent stacks with a state activation per layer.  tests/test_act_numpy_ref.py holds
it to the oracle (oracle/neuralnet.py, oracle/recurrent.py) at 1e-12; the GPU tests of the tanh paths compare against it
where the oracle would be too slow.  The ffLayer functions take the element type (`dt`, float64 unless given): the same
chain in float32 is how a test measures what the format itself costs on its input.

An ffLayer stack is [(W, b)]; a recurrent layer is (s, Ws, W, b, state_act): s [n] or [B, n], Ws = W' [n, n] and state_act
"logistic" / "tanh" for a fullyConnected layer, None, None and None for an ffLayer.  The backward of an activation is
written on its stored output h: h (1 - h) for logistic, 1 - h^2 for tanh."""
import numpy as np


def _sig(z):
    return 1 / (1 + np.exp(-z))


ACT = {"logistic": _sig, "tanh": np.tanh}
DACT = {"logistic": lambda h: h * (1 - h), "tanh": lambda h: 1 - h * h}


def softmax(z):
    e = np.exp(z - z.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


def out_fn(z, out_act):
    return softmax(z) if out_act == "softmax" else _sig(z)


def head(Z, Y, out_act):
    """(dZ, losses) of softmax >>> crossEntropy or logistic >>> squaredError, per row"""
    if out_act == "softmax":
        p = softmax(Z)
        return p * Y.sum(axis=-1, keepdims=True) - Y, -(Y * np.log(p)).sum(axis=-1)
    s = _sig(Z)
    return -2 * (Y - s) * s * (1 - s), ((Y - s) ** 2).sum(axis=-1)


def _cast(ws, dt):
    return [(np.asarray(w, dt), np.asarray(b, dt)) for w, b in ws]


def forward(ws, X, hidden, out_act=None, dt=np.float64):
    """activations [X, a_1, .., a_{L-1}, z_L] for rows X [B, i0]; with out_act, (that list, out_act(z_L))"""
    a = [np.asarray(X, dt)]
    for l, (w, b) in enumerate(_cast(ws, dt)):
        z = a[-1] @ w.T + b
        a.append(z if l == len(ws) - 1 else ACT[hidden](z))
    return a if out_act is None else (a, out_fn(a[-1], out_act))


def grads(ws, X, Y, hidden, out_act, dt=np.float64):
    """([(gW, gb)] summed over the rows, losses [B], gx [B, i0])"""
    ws = _cast(ws, dt)
    a = forward(ws, X, hidden, dt=dt)
    dz, losses = head(a[-1], np.asarray(Y, dt), out_act)
    g = [None] * len(ws)
    for l in range(len(ws) - 1, -1, -1):
        g[l] = (dz.T @ a[l], dz.sum(axis=0))
        dz = dz @ ws[l][0]
        if l > 0:
            dz = dz * DACT[hidden](a[l])
    return g, losses, dz


def sgd(ws, X, Y, rate, hidden, out_act, dt=np.float64):
    g, _, _ = grads(ws, X, Y, hidden, out_act, dt)
    rate = dt(rate)
    return [(w - rate * gw, b - rate * gb) for (w, b), (gw, gb) in zip(_cast(ws, dt), g)]


def online(ws, X, Y, order, rate, hidden, out_act, dt=np.float64):
    """`foldl' trainNetwork` over the rows `order`"""
    ws = _cast(ws, dt)
    for s in order:
        ws = sgd(ws, X[s][None], Y[s][None], rate, hidden, out_act, dt)
    return ws


def induce(ws, X, Y, rate, iters, hidden, out_act, dt=np.float64):
    """(x_iters [B, i0], the last iteration's gradient, losses [B, iters])"""
    x = np.asarray(X, dt).copy()
    Y = np.broadcast_to(np.asarray(Y, dt), (x.shape[0], np.shape(Y)[-1]))
    losses = np.zeros((x.shape[0], iters), dt)
    rate = dt(rate)
    gx = None
    for k in range(iters):
        _, losses[:, k], gx = grads(ws, x, Y, hidden, out_act, dt)
        x = x - rate * gx
    return x, gx, losses


def rnn_forward(layers, X, hidden, out_act):
    """(out [B, T, n_L], per-layer cache (input, z, states [B, T+1, n] or None, output))"""
    X = np.asarray(X, np.float64)
    B, T, _ = X.shape
    a, cache = X, []
    for l, (s, Ws, W, b, sact) in enumerate(layers):
        last = l == len(layers) - 1
        W = np.asarray(W, np.float64)
        Z = a @ W.T + np.asarray(b, np.float64)
        S = None
        if Ws is not None:
            Ws = np.asarray(Ws, np.float64)
            S = np.empty((B, T + 1, W.shape[0]))
            S[:, 0] = np.asarray(s, np.float64)
            for t in range(T):
                Z[:, t] = Z[:, t] + S[:, t] @ Ws.T
                S[:, t + 1] = ACT[sact](Z[:, t])
        out = out_fn(Z, out_act) if last else ACT[hidden](Z)
        cache.append((a, Z, S, out))
        a = out
    return a, cache


def rnn_final_states(cache):
    return [c[2][:, -1] if c[2] is not None else None for c in cache]


def rnn_bptt(layers, X, Y, hidden, out_act):
    """objective sum_b sum_t loss(out_bt, Y_bt): (gs, gWs, gW, gb per layer -- states unbatched --, gx [B, T, i],
    losses [B, T])"""
    _, cache = rnn_forward(layers, X, hidden, out_act)
    dZ, losses = head(cache[-1][1], np.asarray(Y, np.float64), out_act)
    n = len(layers)
    gs, gws, gw, gb = [None] * n, [None] * n, [None] * n, [None] * n
    gx = None
    for l in range(n - 1, -1, -1):
        s, Ws, W, b, sact = layers[l]
        a_in, _, S, _ = cache[l]
        dZ = dZ.copy()
        if Ws is not None:
            Ws = np.asarray(Ws, np.float64)
            h = S[:, 1:]
            for t in range(dZ.shape[1] - 2, -1, -1):
                dZ[:, t] += (dZ[:, t + 1] @ Ws) * DACT[sact](h[:, t])
            gws[l] = np.einsum("btj,btk->jk", dZ, S[:, :-1])
            gs[l] = (dZ[:, 0] @ Ws).sum(axis=0)
        gw[l] = np.einsum("btj,btk->jk", dZ, a_in)
        gb[l] = dZ.sum(axis=(0, 1))
        da = dZ @ np.asarray(W, np.float64)
        if l > 0:
            dZ = da * DACT[hidden](cache[l - 1][3])
        else:
            gx = da
    return gs, gws, gw, gb, gx, losses
