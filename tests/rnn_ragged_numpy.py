"""A masked numpy restatement, in float64, of the recurrent stacks of to_rnn_stack_*_ragged: a batch X [B, T, i] whose
sequence b is steps 0 .. lens[b]-1 of X[b], the rest padding.  Forward, final states (the state after step lens[b]-1) and
BPTT of the masked objective sum_b sum_{t < lens[b]} loss(out_bt, Y_bt), with zeros at padding in out, gx and losses.
Padding is replaced before any arithmetic, so its values (NaN included) reach nothing.

Layers and activations as tests/rnn_numpy.py (logistic states and hidden layers); tests/test_rnn_ragged_numpy_ref.py checks
this file against that one run sequence by sequence."""
import numpy as np

from rnn_numpy import sig, softmax


def mask_of(lens, T):
    lens = np.asarray(lens, np.int64)
    assert lens.ndim == 1 and (lens >= 1).all() and (lens <= T).all()
    return np.arange(T)[None, :] < lens[:, None]   # [B, T]


def forward(layers, X, lens, out_act):
    """(out [B, T, n_L] zero at padding, per-layer cache (input, z, states [B, T+1, n] or None, output), mask)"""
    B, T, _ = np.shape(X)
    m = mask_of(lens, T)
    a = np.where(m[..., None], np.asarray(X, np.float64), 0.0)
    cache = []
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
                S[:, t + 1] = np.where(m[:, t, None], sig(Z[:, t]), S[:, t])   # a finished sequence keeps its state
        out = (softmax(Z) if out_act == "softmax" else sig(Z)) if last else sig(Z)
        out = np.where(m[..., None], out, 0.0)
        cache.append((a, Z, S, out))
        a = out
    return a, cache, m


def final_states(cache):
    return [c[2][:, -1] if c[2] is not None else None for c in cache]


def bptt(layers, X, Y, lens, out_act, loss):
    """(gs, gWs, gW, gb per layer -- states unbatched --, gx [B, T, i], losses [B, T]); gx and losses zero at padding"""
    _, cache, m = forward(layers, X, lens, out_act)
    mk = m[..., None]
    Y = np.where(mk, np.asarray(Y, np.float64), 0.0)
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
    dZ = np.where(mk, dZ, 0.0)
    losses = np.where(m, losses, 0.0)
    n = len(layers)
    gs, gws, gw, gb = [None] * n, [None] * n, [None] * n, [None] * n
    gx = None
    T = m.shape[1]
    for l in range(n - 1, -1, -1):
        s, Ws, W, b = layers[l]
        a_in, Zl, S, _ = cache[l]
        dZ = dZ.copy()
        if Ws is not None:
            Ws = np.asarray(Ws, np.float64)
            h = sig(Zl)   # the state after step t where t is a step of the sequence
            for t in range(T - 2, -1, -1):   # step t hears from step t + 1 only where the sequence has one
                dZ[:, t] += np.where(m[:, t + 1, None], (dZ[:, t + 1] @ Ws) * h[:, t] * (1.0 - h[:, t]), 0.0)
            Sprev = np.where(mk, S[:, :-1], 0.0)
            gws[l] = np.einsum("btj,btk->jk", dZ, Sprev)
            gs[l] = (dZ[:, 0] @ Ws).sum(axis=0)
        gw[l] = np.einsum("btj,btk->jk", dZ, a_in)
        gb[l] = dZ.sum(axis=(0, 1))
        da = dZ @ np.asarray(W, np.float64)
        if l > 0:
            hb = cache[l - 1][3]
            dZ = np.where(mk, da * hb * (1.0 - hb), 0.0)
        else:
            gx = np.where(mk, da, 0.0)
    return gs, gws, gw, gb, gx, losses
