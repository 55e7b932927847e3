"""The step's kernels behind their reduction barriers ("epilogues"): the loss head's target element is fetched
ahead of the barrier through a bounds-checked descriptor (a lane outside the tile's extents reads 0), dz, the losses and the
fused tail's eight values -- computed first -- are stored through descriptors on their outputs (a lane outside stores
nothing); in the generic 16x16 kernel as in the lean head kernels.  The weight-gradient pair's kernel is the parent's (its
part of the change showed no gain, read slower in its job and is not in); its two forms are here so that the whole step
is.  No arithmetic changed, so on the cases of tests/step_epilogue_cases.py (which says what each shape reaches) the
parameters after one and after five steps are

* the fp64 reference's at 1e-5 (tests/act_numpy.py, held to the oracle at 1e-12 by tests/test_act_numpy_ref.py), the bound of
  tests/test_gpu_step_overlap.py, and
* BIT FOR BIT what the parent commit computed on an MI355X: tests/golden/step_epilogue/parent.npz, recorded twice with
  tools/record_step_epilogue.py (both recordings identical).  (About 370 KB, not the few kilobytes first hoped for: a
  parameter set of the 272-wide cases alone is 60 KB.)

What can go wrong is a wrong address (another row's target, a tail value in the wrong column), a lane that should have
been masked reading or writing.  Every case asserts the step's launch count."""
import os

import numpy as np
import pytest

import act_numpy as AN
import step_epilogue_cases as SC

pytestmark = pytest.mark.gpu

RTOL = 1e-5
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "step_epilogue", "parent.npz")


@pytest.fixture(scope="module")
def T():
    from tensor_ops_amd.hipt import HipT
    return HipT(0)


@pytest.fixture(scope="module")
def parent():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def rel_err(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    return np.linalg.norm((got - want).ravel()) / np.linalg.norm(want.ravel())


@pytest.mark.parametrize("case", SC.CASES, ids=[c[0] for c in SC.CASES])
def test_parameters_after_one_and_five_steps(T, parent, case):
    name, rows, i, h, o, out_act, loss, act, launches = case
    got, n = SC.run(T, case)
    print("launches of a step", n)
    assert n == launches
    ws, X, Y = SC.problem(case)
    ref, done = ws, 0
    for steps in SC.STEPS:
        for _ in range(steps - done):
            ref = AN.sgd(ref, X, Y, SC.rate_of(rows), act, out_act)
        done = steps
        want = [ref[0][0], ref[0][1], ref[1][0], ref[1][1]]
        errs = [rel_err(g, w) for g, w in zip(got[steps], want)]
        print("after %d steps, rel_err against fp64:" % steps, errs)
        assert max(errs) < RTOL
        for key, g in zip(SC.keys(case, steps), got[steps]):
            assert g.dtype == np.float32
            assert np.array_equal(g, parent[key]), (key, int(np.sum(g != parent[key])), float(np.max(np.abs(g - parent[key]))))


@pytest.mark.parametrize("out_act,loss", [SC.SM, SC.LG])
@pytest.mark.parametrize("hidden", [40, 136])
def test_rows_beyond_the_batch_are_never_read_as_targets(T, out_act, loss, hidden):
    """17 rows out of buffers of 32 whose other rows are NaN (targets) -- the lanes of rows 17..31 of the second tile are the
    masked ones; a prefetched NaN would reach the row's loss and, through the fused tail (hidden 136), dZ1 and W1.  Losses
    and parameters are finite and equal, bit for bit, to those of the same step on buffers of exactly 17 rows."""
    rows, i, o = 17, 8, 10
    rng = np.random.default_rng(SC.SEED + 1000 + hidden)
    ws = [(0.5 * rng.standard_normal((hidden, i)), 0.5 * rng.standard_normal(hidden)),
          (0.5 * rng.standard_normal((o, hidden)), 0.5 * rng.standard_normal(o))]
    X = rng.uniform(0, 1, size=(32, i))
    Y = np.full((32, o), np.nan)
    Y[:rows] = 0.0
    Y[np.arange(rows), rng.integers(0, o, size=rows)] = 1.0
    out = []
    for n_buf in (rows, 32):
        W, b = [T.put(w) for w, _ in ws], [T.put(v) for _, v in ws]
        x, y = T.put(X[:n_buf], batched=True), T.put(Y[:n_buf], batched=True)
        T.sync()
        n0 = T.stats()["launches"]
        losses = T.stack_minibatch_sgd(W, b, x, y, SC.rate_of(rows), rows, n=rows, out_act=out_act, loss=loss, want_losses=True)
        T.sync()
        launches = T.stats()["launches"] - n0
        out.append([losses.numpy(), W[0].numpy(), b[0].numpy(), W[1].numpy(), b[1].numpy(), launches])
    clean, padded = out
    print("launches of the step", clean[-1], padded[-1])
    assert clean[-1] == padded[-1] == (3 if hidden == 136 else 4)   # forward; head (+ tail) [; dZ1]; the short-K pair
    assert clean[0].shape == (rows,)
    for name, c, p in zip(("losses", "W1", "b1", "W2", "b2"), clean, padded):
        assert np.all(np.isfinite(p)), name
        assert np.array_equal(c, p), name
    want = AN.sgd(ws, X[:rows], Y[:rows], SC.rate_of(rows), "logistic", out_act)
    errs = [rel_err(g, w) for g, w in zip(padded[1:5], [want[0][0], want[0][1], want[1][0], want[1][1]])]
    print("rel_err against fp64:", errs)
    assert max(errs) < RTOL
