"""The two dependent chains taken out of the batched step's launches:

* forward kernel (gemm_t32.hip, eight waves a tile): a wave whose run of K is an odd number of 16-k units no longer pays a DMA
  round trip for the half chunk at its end -- it loads that unit straight into the MFMA fragment layout and runs its eight MFMAs
  while chunk 0 is in flight.  Checked here: products bit-exact on small integers in all four operand layouts at the K values that
  decide which waves have such a unit and how ragged it is, edge tiles, a grid above one round of CUs (four waves, unchanged),
  the fused bias + logistic, the row sums, and non-finite values placed where the unit's masks end.
* loss head (gemm_small.hip): the one-shot instance of two chunks a wave, sixteen-lane reductions by row-local DPP moves.
  Checked here: both heads against tests/closed_form.py at 1e-5 for full and ragged row counts and output widths 10 and 16,
  three launches a step, and the same bits from two runs."""
import ctypes as C

import numpy as np
import pytest

import nonfinite_ref as NF

pytestmark = pytest.mark.gpu

SEED = 0x7e500061
RTOL = 1e-5
INF, NAN = np.float32(np.inf), np.float32(np.nan)


@pytest.fixture(scope="module")
def T():
    from tensor_ops_amd.hipt import HipT
    return HipT(0)


def layout(T, x, trans):
    """the matrix x, row-major or as the transposed view of its column-major copy"""
    return T.transp(T.put(np.ascontiguousarray(x.T))) if trans else T.put(x)


def product(T, a, b, ta, tb):
    return T.gmul(1, 1, 1, layout(T, a, ta), layout(T, b, tb)).numpy()


# K (units of 16; what the eight-wave split makes of it):
#  256 (16: two units a wave, no odd run)    272 (17: wave 7 has one chunk and a register unit)
#  264 (17: the register unit itself ragged, 8 k valid)    784 (49: the step's K, wave 7 has 6 + 1)
#  788 (50: waves 3 and 7 have 6 + 1, wave 7's register unit is a 4-k tail)
KS = [256, 272, 264, 784, 788]
# (M, N): the smallest grid the 32x32-tile route takes (96 tiles), the same with edge tiles in both extents, and a grid above
# one round of 256 CUs (272 tiles: four waves a tile, the form that did not change); the step's own shape once
CASES = [(384, k, 256) for k in KS] + [(368, k, 252) for k in (264, 788)] + [(1088, 784, 256), (1024, 784, 256)]


@pytest.mark.parametrize("ta,tb", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("m,k,n", CASES)
def test_forward_products_bit_exact_on_integers_in_every_layout(T, m, k, n, ta, tb):
    rng = np.random.default_rng(SEED + 2 * ta + tb)
    a = rng.integers(-2, 3, size=(m, k)).astype(np.float32)
    b = rng.integers(-2, 3, size=(k, n)).astype(np.float32)
    got = product(T, a, b, ta, tb)
    want = (a.astype(np.float64) @ b.astype(np.float64)).astype(np.float32)
    assert np.array_equal(got, want), (int(np.sum(got != want)), np.argwhere(got != want)[:4].tolist())


def test_forward_layer_with_bias_and_logistic(T):
    """edge tiles, two waves with a register unit, a 4-k tail: `W x + b` exact on integers, 2e-6 absolute under the logistic"""
    from tensor_ops_amd import hipt
    rows, i, o = 368, 788, 252
    rng = np.random.default_rng(SEED + 11)
    W = rng.integers(-2, 3, (o, i)).astype(np.float32)
    X = rng.integers(-2, 3, (rows, i)).astype(np.float32)
    bb = rng.integers(-3, 4, o).astype(np.float32)
    want = X.astype(np.float64) @ W.T.astype(np.float64) + bb
    dW, dX, db = T.put(W), T.put(X, batched=True), T.put(bb)
    with T.memo():
        z = T.force(T.sumT([T.matVec(dW, dX), db], (o,)))
    assert np.array_equal(z.numpy().reshape(rows, o), want.astype(np.float32))
    with T.memo():
        h = T.force(T.liftT(hipt.logistic_closure, [T.sumT([T.matVec(dW, dX), db], (o,))], key="chains-logistic"))
    err = np.max(np.abs(h.numpy().reshape(rows, o) - 1 / (1 + np.exp(-want))))
    print("max abs error under the logistic:", err)
    assert err < 2e-6


def _flat(tr):
    from tensor_ops_amd import capi
    _, g_ptr, n = tr.flat()
    flat = np.empty(n, dtype=np.float32)
    h = capi.c_tensor()
    d = (C.c_int64 * 1)(n)
    capi.check(capi.lib().to_wrap(C.c_void_p(g_ptr), 0, 1, d, 0, C.byref(h)))
    capi.check(capi.lib().to_download(h, flat.ctypes.data_as(C.c_void_p), flat.nbytes))
    capi.lib().to_release(h)
    return flat


def _split(flat, shapes):
    out, off = [], 0
    for s in shapes:
        n = int(np.prod(s))
        out.append(flat[off:off + n].reshape(s))
        off += (n + 3) // 4 * 4   # (every parameter starts on a 16-byte boundary of the flat buffer)
    return out


def rel_err(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return np.linalg.norm((got - want).ravel()) / np.linalg.norm(want.ravel())


def problem(rng, rows, i, h, o, onehot=True):
    ws = [(0.5 * rng.standard_normal((h, i)), 0.5 * rng.standard_normal(h)),
          (0.5 * rng.standard_normal((o, h)), 0.5 * rng.standard_normal(o))]
    X = rng.uniform(0, 1, size=(rows, i))
    if onehot:
        Y = np.zeros((rows, o))
        Y[np.arange(rows), rng.integers(0, o, size=rows)] = 1.0
    else:
        Y = rng.uniform(0.05, 1.0, (rows, o))
    return ws, X, Y


def test_row_sums_beside_a_register_unit(T):
    """The public route that reaches the 32x32-tile body with row sums: a batch the weight-gradient pair launch does not take
    (272 rows), so `dW1 = dZ1^T X` (256 x 784 over K = 272: 200 tiles, both operands row-contiguous, eight waves, wave 7 with a
    register unit) goes out on its own with `db1` as its row sums.  Without the unit's A elements db1 would be off by 16 / 272
    of itself.  (Which kernel ran is not visible from here: the routing is gemm_t32_applicable's.)"""
    from tensor_ops_amd import tops
    from tests.closed_form import softmax_ce_grads
    rng = np.random.default_rng(SEED + 21)
    ws, X, Y = problem(rng, 272, 784, 256, 10)
    net = tops.genNet([(T.put(w), T.put(b)) for w, b in ws], "actMapLogistic", "actSoftmax")
    tr = tops.Trainer(net, "crossEntropy", 0.01, T.put(X, batched=True), T.put(Y, batched=True), use_graph=False)
    tr.grad()
    want, _ = softmax_ce_grads(X, Y, ws[0][0], ws[0][1], ws[1][0], ws[1][1])
    for name, g, w in zip(("dW1", "db1", "dW2", "db2"), _split(_flat(tr), [w.shape for w in want]), want):
        e = rel_err(g, w)
        print(name, "rel_err", e)
        assert e < RTOL


def tailed(T, arr, tail):
    """arr as a view at the start of a device buffer that goes on with `tail`: what lies right behind the operand"""
    from tensor_ops_amd import capi
    from tensor_ops_amd.hipt import DT
    host = np.concatenate([arr.ravel(), np.asarray(tail, np.float32)])
    base = T.put(host)
    assert base.ptr % 16 == 0
    d = (C.c_int64 * arr.ndim)(*arr.shape)
    h = capi.c_tensor()
    capi.check(capi.lib().to_wrap(C.c_void_p(base.ptr), T.to_dtype, arr.ndim, d, 0, C.byref(h)))
    return DT(h), base


def tailed_layout(T, x, trans, tail):
    v, base = tailed(T, np.ascontiguousarray(x.T) if trans else x, tail)
    return (T.transp(v) if trans else v), (v, base)


@pytest.mark.parametrize("ta,tb", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("m,k,n", [(368, 264, 252), (368, 788, 252)])
def test_poison_at_the_masking_edges_of_the_register_unit(T, m, k, n, ta, tb):
    """Edge tiles and a ragged K (264: the unit has 8 valid k; 788: 4).
    1. +inf and NaN right BEHIND the operands -- for a k-contiguous operand the bytes behind its last row's K extent and the
       row behind M (or N); for a row-contiguous one the k row behind K: the product equals the clean product, bit for bit.
    2. +inf and NaN IN the first elements of the row that follows a row's K extent (k-contiguous: rows r + 1 of A, columns
       c + 1 of B; the last row too): they belong to that row, and IEEE arithmetic says which outputs they reach
       (tests/nonfinite_ref.py) -- every other output equals the clean product.
    Each poisoned run is followed by the clean run of the same shape."""
    rng = np.random.default_rng(SEED + 31 + 2 * ta + tb)
    a = rng.integers(-2, 3, size=(m, k)).astype(np.float32)
    b = rng.integers(-2, 3, size=(k, n)).astype(np.float32)
    clean = (a.astype(np.float64) @ b.astype(np.float64)).astype(np.float32)
    tail = np.tile(np.array([INF, NAN, -INF, NAN], np.float32), 2 * max(m, n, k))[:2 * max(m, n, k) + 64]
    da, keep_a = tailed_layout(T, a, ta, tail)
    db, keep_b = tailed_layout(T, b, tb, tail)
    got = T.gmul(1, 1, 1, da, db).numpy()
    assert np.array_equal(got, clean), ("poison behind the operands", NF.describe(got, clean))
    del da, db, keep_a, keep_b
    assert np.array_equal(product(T, a, b, ta, tb), clean)
    ap, bp = a.copy(), b.copy()
    for r in (0, 37, m - 2):              # (row r + 1 starts where row r's K extent ends)
        ap[r + 1, 0], ap[r + 1, 1] = INF, NAN
    for c in (0, 100, n - 2):
        bp[0, c + 1], bp[1, c + 1] = INF, NAN
    got = product(T, ap, bp, ta, tb)
    want = NF.contract(ap, bp)
    assert NF.same_class_and_value(got, want), ("poison in the next row", NF.describe(got, want))
    fin = np.isfinite(want)
    assert fin.any() and np.array_equal(got[fin], clean[fin])
    assert np.array_equal(product(T, a, b, ta, tb), clean)


HEADS = [("actSoftmax", "crossEntropy"), ("actLogistic", "squaredError")]


@pytest.mark.parametrize("onehot", [True, False])
@pytest.mark.parametrize("o", [10, 16])
@pytest.mark.parametrize("rows", [16, 1000, 1024])
@pytest.mark.parametrize("head,loss", HEADS)
def test_loss_heads_against_the_closed_form(T, head, loss, rows, o, onehot):
    """Gradients against the closed form at 1e-5, the same bits from two runs, and three launches a step.  (At 16 rows the
    third launch is the weight-gradient pair's short-K form, one wave per 16x16 tile: launch_gemm_small_pair.)"""
    from tensor_ops_amd import tops
    from tests.closed_form import logistic_se_grads, softmax_ce_grads
    rng = np.random.default_rng(SEED + 40 + rows + o)
    ws, X, Y = problem(rng, rows, 784, 256, o, onehot)
    net = tops.genNet([(T.put(w), T.put(b)) for w, b in ws], "actMapLogistic", head)
    tr = tops.Trainer(net, loss, 0.01, T.put(X, batched=True), T.put(Y, batched=True), use_graph=False)
    launches = tr.launches_per_step
    print("launches_per_step", launches)
    tr.grad()
    first = _flat(tr).copy()
    f = softmax_ce_grads if loss == "crossEntropy" else logistic_se_grads
    want, _ = f(X, Y, ws[0][0], ws[0][1], ws[1][0], ws[1][1])
    for name, g, w in zip(("dW1", "db1", "dW2", "db2"), _split(first, [w.shape for w in want]), want):
        e = rel_err(g, w)
        print(name, "rel_err", e)
        assert e < RTOL
    tr.grad()
    assert np.array_equal(first.view(np.uint32), _flat(tr).view(np.uint32)), "two runs of the same input differ"
    assert launches == 3
