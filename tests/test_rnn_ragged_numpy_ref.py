"""CPU: the masked restatement of tests/rnn_ragged_numpy.py against tests/rnn_numpy.py run sequence by sequence on
X[b:b+1, :lens[b]] and summed; and NaN in the padding changes no bit of it."""
import numpy as np
import pytest

import rnn_numpy as RN
import rnn_ragged_numpy as RR

CASES = [  # (i, [(n, stateful)], out_act, loss)
    (2, [(3, True)], "logistic", "squaredError"),
    (3, [(4, True), (5, False), (2, True)], "softmax", "crossEntropy"),
    (5, [(6, False), (7, True)], "softmax", "crossEntropy"),
    (9, [(37, True), (30, True), (11, False)], "softmax", "crossEntropy"),
]
LENS = [3, 1, 5, 5, 2, 4, 1]
T = 5


def make(rng, i, spec):
    layers, prev = [], i
    for n, st in spec:
        W, b = 0.5 * rng.standard_normal((n, prev)), 0.5 * rng.standard_normal(n)
        s, ws = (0.5 * rng.standard_normal(n), 0.5 * rng.standard_normal((n, n))) if st else (None, None)
        layers.append((s, ws, W, b))
        prev = n
    return layers


def problem(case):
    i, spec, out_act, loss = case
    rng = np.random.default_rng(i * 7 + len(spec))
    layers = make(rng, i, spec)
    B = len(LENS)
    X = rng.uniform(-1, 1, (B, T, i))
    Y = rng.uniform(0.1, 0.9, (B, T, spec[-1][0]))
    return layers, X, Y, out_act, loss


def close(a, b):
    return np.allclose(a, b, rtol=1e-12, atol=1e-13)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "i%d_L%d" % (c[0], len(c[1])))
def test_masked_equals_sequence_by_sequence(case):
    layers, X, Y, out_act, loss = problem(case)
    out, cache, _ = RR.forward(layers, X, LENS, out_act)
    fin = RR.final_states(cache)
    gs, gws, gw, gb, gx, losses = RR.bptt(layers, X, Y, LENS, out_act, loss)
    n = len(layers)
    acc = {k: [0.0] * n for k in ("gs", "gws", "gw", "gb")}
    for q, ln in enumerate(LENS):
        xo, co = RN.forward(layers, X[q:q + 1, :ln], out_act)
        assert close(out[q, :ln], xo[0]) and np.array_equal(out[q, ln:], np.zeros_like(out[q, ln:]))
        for l, st in enumerate(RN.final_states(co)):
            assert (st is None) == (fin[l] is None)
            if st is not None:
                assert close(fin[l][q], st[0])
        g = RN.bptt(layers, X[q:q + 1, :ln], Y[q:q + 1, :ln], out_act, loss)
        for k, v in zip(("gs", "gws", "gw", "gb"), g[:4]):
            for l in range(n):
                if v[l] is not None:
                    acc[k][l] = acc[k][l] + v[l]
        assert close(gx[q, :ln], g[4][0]) and not gx[q, ln:].any()
        assert close(losses[q, :ln], g[5][0]) and not losses[q, ln:].any()
    for k, got in zip(("gs", "gws", "gw", "gb"), (gs, gws, gw, gb)):
        for l in range(n):
            assert (got[l] is None) == (isinstance(acc[k][l], float))
            if got[l] is not None:
                assert close(got[l], acc[k][l]), (k, l)


@pytest.mark.parametrize("case", CASES[:2], ids=lambda c: "i%d_L%d" % (c[0], len(c[1])))
def test_nan_padding_changes_nothing(case):
    layers, X, Y, out_act, loss = problem(case)
    m = RR.mask_of(LENS, T)
    Xn, Yn = X.copy(), Y.copy()
    Xn[~m] = np.nan
    Yn[~m] = np.nan
    a = RR.bptt(layers, X, Y, LENS, out_act, loss)
    b = RR.bptt(layers, Xn, Yn, LENS, out_act, loss)
    for u, v in zip(a[:4], b[:4]):
        for p, q in zip(u, v):
            assert (p is None and q is None) or (np.isfinite(q).all() and np.array_equal(p, q))
    assert np.array_equal(a[4], b[4]) and np.array_equal(a[5], b[5])
    oa, ca, _ = RR.forward(layers, X, LENS, out_act)
    ob, cb, _ = RR.forward(layers, Xn, LENS, out_act)
    assert np.array_equal(oa, ob) and np.isfinite(ob).all()
    for p, q in zip(RR.final_states(ca), RR.final_states(cb)):
        assert (p is None and q is None) or np.array_equal(p, q)


def test_all_lengths_T_is_the_dense_restatement():
    layers, X, Y, out_act, loss = problem(CASES[1])
    full = [T] * len(LENS)
    a = RR.bptt(layers, X, Y, full, out_act, loss)
    b = RN.bptt(layers, X, Y, out_act, loss)
    for u, v in zip(a[:4], b[:4]):
        for p, q in zip(u, v):
            assert (p is None and q is None) or close(p, q)
    assert close(a[4], b[4]) and close(a[5], b[5])
