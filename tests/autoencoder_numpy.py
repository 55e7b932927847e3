"""AutoEncoder.hs restated in numpy, in float64 unless asked otherwise: what to_autoencoder_stack_* compute.  An
encoder / decoder pair is one list of (W, b) in input-to-output order whose first n_enc entries are the encoder; layer l
applies `hidden` except for the encoder's output (`code_act`) and the last layer (`out_act`); the target of a row is the row
itself.  The (out_act, loss) pairs: softmax goes with crossEntropy, logistic / tanh / identity with squaredError
= sum (a - x)^2, dz = 2 (a - x) act'(a) with act' written on the output a.  An identity layer has no activation in the
forward pass and no act' factor in the backward pass.  tests/test_autoencoder_numpy_ref.py holds this to
oracle/autoencoder.py at 1e-12; tests/test_gpu_autoencoder.py compares the GPU entries against it."""
import numpy as np

import act_numpy as AN

ACT = dict(AN.ACT, identity=lambda z: z)
DACT = dict(AN.DACT, identity=lambda h: np.ones_like(h))
HIDDEN = ["logistic", "tanh"]
CODE = ["logistic", "tanh", "identity"]
PAIRS = {"softmax": "crossEntropy", "logistic": "squaredError", "tanh": "squaredError", "identity": "squaredError"}


def acts(n_layers, n_enc, hidden, code_act):
    a = [hidden] * n_layers
    a[n_enc - 1] = code_act
    return a


def out_fn(z, out_act):
    return AN.softmax(z) if out_act == "softmax" else ACT[out_act](z)


def head(Z, X, out_act):
    """(dZ, losses, a) per row"""
    if out_act == "softmax":
        p = AN.softmax(Z)
        return p * X.sum(axis=-1, keepdims=True) - X, -(X * np.log(p)).sum(axis=-1), p
    a = ACT[out_act](Z)
    return 2 * (a - X) * DACT[out_act](a), ((a - X) ** 2).sum(axis=-1), a


def forward(ws, n_enc, X, hidden, code_act, dt=np.float64):
    """[X, a_1, .., a_{L-1}, z_L]"""
    ws = AN._cast(ws, dt)
    k = acts(len(ws), n_enc, hidden, code_act)
    a = [np.asarray(X, dt)]
    for l, (w, b) in enumerate(ws):
        z = a[-1] @ w.T + b
        a.append(z if l == len(ws) - 1 else ACT[k[l]](z))
    return a


def encode(ws, n_enc, X, hidden, code_act, dt=np.float64):
    return forward(ws, n_enc, X, hidden, code_act, dt)[n_enc]


def decode(ws, n_enc, C, hidden, out_act, dt=np.float64):
    a = np.asarray(C, dt)
    dec = AN._cast(ws[n_enc:], dt)
    for l, (w, b) in enumerate(dec):
        z = a @ w.T + b
        a = out_fn(z, out_act) if l == len(dec) - 1 else ACT[hidden](z)
    return a


def run(ws, n_enc, X, hidden, code_act, out_act, dt=np.float64):
    """(code, recon, losses): encode, encodeDecode, testEncoder per row"""
    a = forward(ws, n_enc, X, hidden, code_act, dt)
    _, losses, recon = head(a[-1], a[0], out_act)
    return a[n_enc], recon, losses


def grads(ws, n_enc, X, hidden, code_act, out_act, dt=np.float64):
    """([(gW, gb)] summed over the rows -- encGrad --, losses [B], dz_L)"""
    ws = AN._cast(ws, dt)
    k = acts(len(ws), n_enc, hidden, code_act)
    a = forward(ws, n_enc, X, hidden, code_act, dt)
    dz, losses, _ = head(a[-1], a[0], out_act)
    dzL = dz
    g = [None] * len(ws)
    for l in range(len(ws) - 1, -1, -1):
        g[l] = (dz.T @ a[l], dz.sum(axis=0))
        if l > 0:
            dz = (dz @ ws[l][0]) * DACT[k[l - 1]](a[l])
    return g, losses, dzL


def sgd(ws, n_enc, X, rate, hidden, code_act, out_act, dt=np.float64):
    """trainEncoder on the rows of X, the gradient summed over them"""
    g, _, _ = grads(ws, n_enc, X, hidden, code_act, out_act, dt)
    rate = dt(rate)
    return [(w - rate * gw, b - rate * gb) for (w, b), (gw, gb) in zip(AN._cast(ws, dt), g)]
