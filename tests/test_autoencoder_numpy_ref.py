"""CPU: the numpy restatement of tests/autoencoder_numpy.py (what tests/test_gpu_autoencoder.py compares the
to_autoencoder_stack_* entries against) agrees with oracle/autoencoder.py -- encode, decode, encodeDecode, testEncoder,
encGrad summed over the rows, and one trainEncoder step -- in fp64 at 1e-12, for every (hidden, code, pair) combination, on
[12, 7, 4, 6, 12] with a two-layer encoder and on [9, 3, 9]."""
import numpy as np
import pytest

import autoencoder_numpy as AEN
from oracle import ad, autoencoder as AE, neuralnet as NN
from oracle.tensor import OTensor

O = OTensor(np.float64)
TOL = 1e-12
OACT = {"logistic": NN.actLogistic, "tanh": lambda: NN.actMap(ad.tanh), "softmax": NN.actSoftmax}
OLOSS = {"crossEntropy": NN.crossEntropy, "squaredError": NN.squaredError}
STACKS = [([12, 7, 4, 6, 12], 2), ([9, 3, 9], 1)]
COMBOS = [(h, c, o) for h in AEN.HIDDEN for c in AEN.CODE for o in AEN.PAIRS]


def close(a, b, tol=TOL):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    assert np.linalg.norm(a - b) <= tol * max(np.linalg.norm(b), 1e-300)


def oracle_net(ws, names):
    """ffLayer *~ act per layer, chained by ~*~; "identity" is the bare ffLayer"""
    net = None
    for (w, b), name in zip(ws, names):
        lay = NN.ffLayer(w, b)
        if name != "identity":
            lay = NN.net_then(lay, OACT[name]())
        net = lay if net is None else NN.seq_net(net, lay)
    return net


def oracle_encoder(ws, n_enc, hidden, code_act, out_act):
    names = AEN.acts(len(ws), n_enc, hidden, code_act)
    names[-1] = out_act
    return AE.Encoder(oracle_net(ws[:n_enc], names[:n_enc]), oracle_net(ws[n_enc:], names[n_enc:]))


def problem(sizes, B, seed, out_act):
    rng = np.random.default_rng(seed)
    ws = [(0.5 * rng.standard_normal((o, i)), 0.5 * rng.standard_normal(o)) for i, o in zip(sizes[:-1], sizes[1:])]
    X = rng.uniform(0.05, 0.95, (B, sizes[0]))
    if out_act == "softmax":
        X = X / X.sum(axis=1, keepdims=True)
    elif out_act != "logistic":
        X = 2 * X - 1
    return ws, X


def test_the_24_combinations_are_all_there():
    assert len(COMBOS) == 24 and len(set(COMBOS)) == 24


@pytest.mark.parametrize("sizes,n_enc", STACKS, ids=lambda v: "-".join(map(str, v)) if isinstance(v, list) else str(v))
@pytest.mark.parametrize("hidden,code_act,out_act", COMBOS, ids=lambda v: v)
def test_autoencoder_matches_oracle(sizes, n_enc, hidden, code_act, out_act):
    B = 3
    ws, X = problem(sizes, B, 0xae + len(sizes), out_act)
    e = oracle_encoder(ws, n_enc, hidden, code_act, out_act)
    loss = OLOSS[AEN.PAIRS[out_act]]()
    code, recon, losses = AEN.run(ws, n_enc, X, hidden, code_act, out_act)
    dec = AEN.decode(ws, n_enc, code, hidden, out_act)
    for r in range(B):
        close(code[r], AE.encode(O, e, X[r]))
        close(AEN.encode(ws, n_enc, X, hidden, code_act)[r], AE.encode(O, e, X[r]))
        close(recon[r], AE.encodeDecode(O, e, X[r]))
        close(dec[r], AE.decode(O, e, AE.encode(O, e, X[r])))
        close(losses[r], AE.testEncoder(O, loss, e, X[r]))
    # encGrad summed over the rows
    g, g_losses, _ = AEN.grads(ws, n_enc, X, hidden, code_act, out_act)
    close(g_losses, losses)
    want = None
    for r in range(B):
        g_e, g_d = AE.encGrad(O, loss, X[r], e)
        flat = [np.asarray(a, np.float64) for a in list(g_e) + list(g_d)]
        want = flat if want is None else [a + b for a, b in zip(want, flat)]
    for l, (gw, gb) in enumerate(g):
        close(gw, want[2 * l])
        close(gb, want[2 * l + 1])
    # one trainEncoder step is the restatement's sgd on that row
    e2 = AE.trainEncoder(O, loss, 0.3, X[1], e)
    new = list(e2.enc.params) + list(e2.dec.params)
    for l, (w, b) in enumerate(AEN.sgd(ws, n_enc, X[1:2], 0.3, hidden, code_act, out_act)):
        close(w, new[2 * l])
        close(b, new[2 * l + 1])
        assert not np.array_equal(w, ws[l][0])
