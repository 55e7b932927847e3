"""The step's kernels take their hot arguments as leading scalars that the dispatcher preloads into registers:
the forward kernel's strides became 32-bit and its two shifts and the chunk depth share one word, its tile grid is derived
from M and N in the kernel; the loss head takes the trivial tile map only and constant k strides; the weight-gradient pair
packs the tile order into n1's word and asks for its operands' members by hand.  A mis-packed or mis-ordered argument is a
workgroup on the wrong tile or an operand read through the wrong member, so, on the smallest shapes that reach each path:

* forward route (eight-wave form: 96..512 tiles of 32 x 32, K >= 256), products bit-exact on small integers (fp32 sums of
  integers this small are exact), K = 272 = 17 units of 16 (odd runs: the register unit), all four operand layouts, on
  320 x 320, 330 x 320 (ragged M; with a row-contiguous A -- M no multiple of 4 -- the plan keeps the product off this kernel and
  it must still be right), 3200 x 32 and 32 x 3200 (XCD grids 8 x 1 and 1 x 8: lgm = 3 / lgn = 3 in the packed word), 256 x 416 and
  416 x 256; and operands that are slices of wider buffers (a base pointer that is not the allocation's).  The library's views are
  `transp` and leading-index slices: it makes no view whose row stride differs from the row's extent, so that case cannot
  be put to it, and the 32-bit strides with stride != extent are exercised by no GPU test (NOT DONE; the launcher's predicate
  for them is tested on the host, tests/test_step_preload.py).
  What this test cannot see: the product build has no counter or switch that names the kernel a "small" launch went to
  (gemm_t32's kernels are entered from inside that family, launch_gemm_small -> gemm_t32_applicable), so a shape that
  t32_fill quietly refused would be computed by gemm_small's generic kernel and still pass here.  A mis-packed argument on
  the route taken is caught; a silent fall-back -- lost speed, right answer -- is not: that shows in the kernel names of a
  profile (profiles/README.md) only.
* whole step through to_fflayer_stack_grad / to_fflayer_stack_sgd, launch counts asserted: 160 -> 96 -> 10 and 96 -> 160 -> 10 at
  720 and 1024 rows (weight-gradient grids 3 x 5 and 5 x 3, both ends of the one-shot pair's range of K), 784 -> 256 -> 10 at 1024
  rows, a 16-output head (still one column of tiles: the lean kernel) and a 17-output head (two columns: the generic kernel),
  logistic and tanh hidden layers.  Gradients and updated parameters against the C oracle (logistic; oracle/hmat.py) or its
  numpy restatement (tanh; tests/act_numpy.py, held to the oracle at 1e-12 by tests/test_act_numpy_ref.py) at the 1e-5 of
  tests/test_gpu_batch_rule.py."""
import numpy as np
import pytest

import act_numpy as AN

pytestmark = pytest.mark.gpu

SEED = 0x7e500093
RTOL = 1e-5
K = 272


@pytest.fixture(scope="module")
def T():
    from tensor_ops_amd.hipt import HipT
    return HipT(0)


def rel_err(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    return np.linalg.norm((got - want).ravel()) / np.linalg.norm(want.ravel())


def _operand(T, x, transposed, sliced):
    """x [r][c] on the device: contiguous, or a transposed view of its transposed copy; `sliced`: as the second of two
    matrices in one buffer"""
    src = np.ascontiguousarray(x.T) if transposed else x
    if sliced:
        d = T.slice(T.put(np.stack([np.full_like(src, 7.0), src])), (1,))
    else:
        d = T.put(src)
    return T.transp(d) if transposed else d


FORWARD = [(320, 320), (330, 320), (3200, 32), (32, 3200), (256, 416), (416, 256)]


@pytest.mark.parametrize("ta,tb", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("m,n,sliced", [(m, n, False) for m, n in FORWARD] + [(320, 320, True), (416, 256, True)])
def test_forward_route_bit_exact_on_integers(T, m, n, sliced, ta, tb):
    assert T.gemm_route(m, K, n, a_transposed=bool(ta), b_transposed=bool(tb))["families"] == ["small"]
    tiles = ((m + 31) // 32) * ((n + 31) // 32)
    assert 96 <= tiles <= 256 and K >= 256 and (K // 16) % 2 == 1      # one round of eight-wave tiles, an odd number of units
    rng = np.random.default_rng(SEED + 1000 * m + 10 * n + 2 * ta + tb)
    a = rng.integers(-2, 3, size=(m, K)).astype(np.float32)
    b = rng.integers(-2, 3, size=(K, n)).astype(np.float32)
    got = T.gmul(1, 1, 1, _operand(T, a, ta, sliced), _operand(T, b, tb, sliced)).numpy()
    want = (a.astype(np.float64) @ b.astype(np.float64)).astype(np.float32)
    assert np.array_equal(got, want), (int(np.sum(got != want)), np.argwhere(got != want)[:4].tolist())


def problem(rng, rows, sizes):
    ws = [(0.5 * rng.standard_normal((o, i)), 0.5 * rng.standard_normal(o)) for i, o in zip(sizes[:-1], sizes[1:])]
    X = rng.uniform(0, 1, size=(rows, sizes[0]))
    Y = np.zeros((rows, sizes[-1]))
    Y[np.arange(rows), rng.integers(0, sizes[-1], size=rows)] = 1.0
    return ws, X, Y


def reference(ws, X, Y, hidden):
    """[(dW, db)] per layer, summed over the rows"""
    if hidden == "logistic":
        from oracle import hmat
        (dW1, db1, dW2, db2), _ = hmat.batched_grads(X, Y, ws[0][0], ws[0][1], ws[1][0], ws[1][1], recompute=False)
        return [(dW1, db1), (dW2, db2)]
    g, _, _ = AN.grads(ws, X, Y, hidden, "softmax")
    return g


# (sizes, rows, launches of a step: forward; loss head + dZ1; the weight-gradient pair -- or None where the count is not this
# change's business).  A hidden layer of 96 is six 16-k chunks, below the eight the fused tail needs: dZ1 is a launch of its
# own, four in all (tests/test_gpu_step_prologue.py) -- still ONE pair launch.  A 17-output head is two columns of 16 x 16
# tiles: not the lean head kernel.
STEPS = [([160, 96, 10], 720, 4), ([160, 96, 10], 1024, 4), ([96, 160, 10], 720, 3), ([96, 160, 10], 1024, 3),
         ([784, 256, 10], 1024, 3), ([96, 160, 16], 720, 3), ([96, 160, 17], 720, None)]


@pytest.mark.parametrize("hidden", ["logistic", "tanh"])
@pytest.mark.parametrize("sizes,rows,launches", STEPS, ids=lambda v: "-".join(map(str, v)) if isinstance(v, list) else str(v))
def test_whole_step_against_the_oracle(T, sizes, rows, launches, hidden):
    rng = np.random.default_rng(SEED + rows + 7 * sizes[1] + sizes[2])
    ws, X, Y = problem(rng, rows, sizes)
    want = reference(ws, X, Y, hidden)
    W, b = [T.put(w) for w, _ in ws], [T.put(v) for _, v in ws]
    x, y = T.put(X, batched=True), T.put(Y, batched=True)
    gW, gB = T.stack_grad(W, b, x, y, "softmax", "crossEntropy", hidden_act=hidden)[:2]
    errs = [rel_err(g.numpy(), w) for g, (w, _) in zip(gW, want)] + [rel_err(g.numpy(), w) for g, (_, w) in zip(gB, want)]
    print("gradients, rel_err", errs)
    assert max(errs) < RTOL
    rate = 0.02
    T.stack_sgd(W, b, x, y, rate, "softmax", "crossEntropy", hidden_act=hidden)
    errs = [max(rel_err(dw.numpy(), w - rate * gw), rel_err(db.numpy(), v - rate * gb))
            for (w, v), (gw, gb), dw, db in zip(ws, want, W, b)]
    print("updated parameters, rel_err", errs)
    assert max(errs) < RTOL
    T.sync()
    n0 = T.stats()["launches"]
    T.stack_sgd(W, b, x, y, rate, "softmax", "crossEntropy", hidden_act=hidden)
    T.sync()
    n = T.stats()["launches"] - n0
    print("launches of a step", n)
    if launches is not None:
        assert n == launches
