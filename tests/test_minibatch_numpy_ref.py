"""tests/minibatch_numpy.py against tests/act_numpy.py at its two ends, and the ctypes table against the header for the two
entries of the one-call minibatch SGD.  No GPU."""
import os
import re

import numpy as np
import pytest

import act_numpy as AN
import minibatch_numpy as MN


def problem(sizes, N, seed, out_act):
    rng = np.random.default_rng(seed)
    ws = [(rng.standard_normal((o, i)) / np.sqrt(i), 0.5 * rng.standard_normal(o)) for i, o in zip(sizes[:-1], sizes[1:])]
    X = rng.uniform(-1, 1, (N, sizes[0]))
    Y = rng.uniform(0.05, 0.95, (N, sizes[-1]))
    if out_act == "softmax":
        Y = Y / Y.sum(axis=1, keepdims=True)
    return ws, X, Y


@pytest.mark.parametrize("hidden", ["logistic", "tanh"])
@pytest.mark.parametrize("out_act", ["softmax", "logistic"])
def test_both_ends_are_act_numpy(hidden, out_act):
    ws, X, Y = problem([7, 5, 3], 23, 0x3b, out_act)
    order = np.random.default_rng(1).integers(0, 23, 17)       # with repeats
    got, losses = MN.minibatch_sgd(ws, X, Y, order, 1, 0.1, hidden, out_act)
    want = AN.online(ws, X, Y, order, 0.1, hidden, out_act)
    for (w, b), (ww, wb) in zip(got, want):
        assert np.array_equal(w, ww) and np.array_equal(b, wb)
    got, losses = MN.minibatch_sgd(ws, X, Y, order, len(order), 0.1, hidden, out_act)
    want = AN.sgd(ws, X[order], Y[order], 0.1, hidden, out_act)
    for (w, b), (ww, wb) in zip(got, want):
        assert np.array_equal(w, ww) and np.array_equal(b, wb)
    assert np.array_equal(losses, AN.grads(ws, X[order], Y[order], hidden, out_act)[1])
    # a minibatch larger than the sample count is one short batch
    again, _ = MN.minibatch_sgd(ws, X, Y, order, 100, 0.1, hidden, out_act)
    assert all(np.array_equal(a[0], g[0]) for a, g in zip(again, got))


def test_short_tail_and_reconstruction():
    assert MN.batches(10, 4) == [(0, 4), (4, 8), (8, 10)] and MN.batches(8, 4) == [(0, 4), (4, 8)]
    ws, X, _ = problem([6, 4, 6], 11, 0x51, "logistic")
    order = np.arange(11)[::-1]
    a, la = MN.minibatch_sgd(ws, X, None, order, 4, 0.2, "logistic", "logistic")
    b, lb = MN.minibatch_sgd(ws, X, X.copy(), order, 4, 0.2, "logistic", "logistic")
    assert all(np.array_equal(p[0], q[0]) and np.array_equal(p[1], q[1]) for p, q in zip(a, b)) and np.array_equal(la, lb)
    # three chained steps by hand
    want = ws
    for rows in (order[0:4], order[4:8], order[8:11]):
        want = AN.sgd(want, X[rows], X[rows], 0.2, "logistic", "logistic")
    assert all(np.array_equal(p[0], q[0]) for p, q in zip(a, want))


def test_ctypes_table_holds_both_entries_with_the_headers_arity(repo_root):
    from tensor_ops_amd import capi
    text = open(os.path.join(repo_root, "include", "tensorops_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("to_fflayer_stack_minibatch_sgd", "to_set_minibatch_stage_bytes"):
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, text)
        assert m, name + " is not declared in the header"
        assert name in capi.SIGNATURES, name
        assert len(capi.SIGNATURES[name]) == len(m.group(1).split(",")), name
    assert len(capi.SIGNATURES["to_fflayer_stack_minibatch_sgd"]) == 13
    assert len(capi.SIGNATURES["to_set_minibatch_stage_bytes"]) == 2
