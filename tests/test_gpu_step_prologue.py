"""The step kernels after their prologues were cut down to one scalar round trip: the argument blocks were
reordered (every instance of gemm_t32.hip / gemm_small.hip reads them) and the workgroup -> tile maps divide by
multiply-high with reciprocals planned on the host.  What can go wrong is a workgroup on the wrong tile or an operand read
through the wrong member, so:

* forward route (family asserted through the route query, the kernel by gemm_t32_applicable's bounds): products bit-exact
  on small integers, all four operand layouts, on a
  tile grid whose count is no multiple of 8 (11 x 9, a 4 x 2 grid of XCD rectangles of two widths), ragged in both extents,
  K an odd number of 16-k units -- and 992 x 788 x 252 (31 x 8 tiles, an 8 x 1 grid);
* loss head: 16 and 48 rows (one and three 16-row tiles, tile map of divisor 1) against the closed form;
* weight-gradient pair: the step's network at 1024, 1000, 720 and 16 rows and two networks whose dW1 grid is 3 x 5 and 5 x 3
  tiles (15: below the XCD-aware order's threshold, row-major map with divisor 5 / 3) at 720 and 16 rows, against the fp64
  oracle; the launch count of every step asserted (three; four where a hidden layer of 96 cannot fuse the tail);
* the whole step at 1024 rows (gradients and updated parameters) against the fp64 oracle at 1e-5."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = 0x7e500071
RTOL = 1e-5


@pytest.fixture(scope="module")
def T():
    from tensor_ops_amd.hipt import HipT
    return HipT(0)


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


# (M, K, N).  340 x 272 x 284: 11 x 9 = 99 tiles, the last row block 20 rows and the last column block 28 columns deep,
# K = 17 units of 16 (wave 7 has a register unit).  992 x 788 x 252: 31 x 8 tiles; the plan runs K = 784 there, 49 units.
FORWARD = [(340, 272, 284), (992, 788, 252)]


@pytest.mark.parametrize("ta,tb", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("m,k,n", FORWARD)
def test_forward_route_bit_exact_on_integers_in_every_layout(T, m, k, n, ta, tb):
    # the plan record names the family: one launch of "small", inside which grids of 96..512 tiles of 32 x 32 with
    # 256 <= K <= 8192 go to the DMA-fed kernel of gemm_t32.hip (gemm_t32_applicable; "t32" as a family of its own only
    # exists under a development build's TOPS_T32_FIRST)
    # (K = 788 is no multiple of 16: the plan runs K = 784 there and adds the 4-k tail in a second, tiny launch)
    want_route = ["small"] if k % 16 == 0 else ["small", "naive"]
    assert T.gemm_route(m, k, n, a_transposed=bool(ta), b_transposed=bool(tb))["families"] == want_route
    tiles = ((m + 31) // 32) * ((n + 31) // 32)
    assert 96 <= tiles <= 256 and tiles % 8 != 0 or (m, k, n) == (992, 788, 252)
    assert 256 <= k <= 8192 and k % 4 == 0 and n % 4 == 0 and m % 4 == 0
    rng = np.random.default_rng(SEED + 2 * ta + tb)
    a = rng.integers(-2, 3, size=(m, k)).astype(np.float32)
    b = rng.integers(-2, 3, size=(k, n)).astype(np.float32)
    da = T.transp(T.put(np.ascontiguousarray(a.T))) if ta else T.put(a)
    db = T.transp(T.put(np.ascontiguousarray(b.T))) if tb else T.put(b)
    got = T.gmul(1, 1, 1, da, db).numpy()
    want = (a.astype(np.float64) @ b.astype(np.float64)).astype(np.float32)
    assert np.array_equal(got, want), (int(np.sum(got != want)), np.argwhere(got != want)[:4].tolist())


def problem(rng, rows, i, h, o):
    ws = [(0.5 * rng.standard_normal((h, i)), 0.5 * rng.standard_normal(h)),
          (0.5 * rng.standard_normal((o, h)), 0.5 * rng.standard_normal(o))]
    X = rng.uniform(0, 1, size=(rows, i))
    Y = np.zeros((rows, o))
    Y[np.arange(rows), rng.integers(0, o, size=rows)] = 1.0
    return ws, X, Y


@pytest.mark.parametrize("rows", [16, 48])
@pytest.mark.parametrize("head,loss", [("actSoftmax", "crossEntropy"), ("actLogistic", "squaredError")])
def test_loss_head_against_the_closed_form(T, head, loss, rows):
    from tensor_ops_amd import tops
    from tests.closed_form import logistic_se_grads, softmax_ce_grads
    rng = np.random.default_rng(SEED + 40 + rows)
    ws, X, Y = problem(rng, rows, 784, 256, 10)
    net = tops.genNet([(T.put(w), T.put(b)) for w, b in ws], "actMapLogistic", head)
    tr = tops.Trainer(net, loss, 0.01, T.put(X, batched=True), T.put(Y, batched=True), use_graph=False)
    launches = tr.launches_per_step
    print("launches_per_step", launches)
    tr.grad()
    f = softmax_ce_grads if loss == "crossEntropy" else logistic_se_grads
    want, _ = f(X, Y, ws[0][0], ws[0][1], ws[1][0], ws[1][1])
    for name, g, w in zip(("dW1", "db1", "dW2", "db2"), _split(_flat(tr), [w.shape for w in want]), want):
        e = rel_err(g, w)
        print(name, "rel_err", e)
        assert e < RTOL
    # (48 rows: K = 48 > 32 puts dW1 on 32x32 tiles, which the pair launch's short-K form -- one wave per 16x16 tile -- does not
    #  take, and its one-shot form starts at 705 rows: the two weight gradients leave one by one, four launches)
    assert launches == (3 if rows == 16 else 4)


def _step_against_the_oracle(T, ws, X, Y):
    """gradients, then the updated parameters, against the fp64 oracle; the step's launch count"""
    from oracle import hmat
    from tensor_ops_amd import tops
    want, _ = hmat.batched_grads(X, Y, ws[0][0], ws[0][1], ws[1][0], ws[1][1], recompute=False)
    net = tops.genNet([(T.put(w), T.put(b)) for w, b in ws], "actMapLogistic", "actSoftmax")
    tr = tops.Trainer(net, "crossEntropy", 0.02, T.put(X, batched=True), T.put(Y, batched=True))
    tr.grad()
    launches = tr.launches_per_step
    print("launches_per_step", launches)
    shapes = [ws[0][0].shape, ws[0][1].shape, ws[1][0].shape, ws[1][1].shape]
    for name, g, w in zip(("dW1", "db1", "dW2", "db2"), _split(_flat(tr), shapes), want):
        e = rel_err(g, w)
        print(name, "rel_err", e)
        assert e < RTOL
    tr.apply()
    for name, p, w0, g in zip(("W1", "b1", "W2", "b2"), tr.net.params, [ws[0][0], ws[0][1], ws[1][0], ws[1][1]], want):
        e = rel_err(p.numpy(), w0 - 0.02 * g)
        print(name, "updated, rel_err", e)
        assert e < RTOL
    return launches


@pytest.mark.parametrize("batch", [1024, 1000, 720, 16])
def test_weight_gradient_pair_and_the_whole_step_on_the_step_network(T, batch):
    """784 -> 256 -> 10 (tests/test_gpu_step_overlap.py's networks, and fewer rows): dW1 on 8 x 25 tiles.  1024 rows is the
    whole step of the benchmark."""
    import bench
    ws, X, Y = bench.synth(3, batch)
    assert _step_against_the_oracle(T, ws, X, Y) == 3   # forward; loss head + dZ1; the weight-gradient pair


# (inputs, hidden, launches a step).  96 x 160 and 160 x 96 weights: dW1 = dZ1^T X on 3 x 5 and on 5 x 3 tiles of 32 x 32 -- 15, below
# the XCD-aware order's threshold: the row-major map with divisor 5 / 3.  A hidden layer of 160 is ten 16-k chunks: the loss
# head fuses the tail and the step is three launches (forward; loss head + dZ1; the weight-gradient pair).  A hidden layer of
# 96 is six, below the eight the fused tail needs (gemm_small_fuses_tail): dZ1 is a launch of its own, four in all -- a count
# that still says the two weight gradients left as ONE pair launch (apart they would make five).
SMALL_NETS = [(160, 96, 4), (96, 160, 3)]


@pytest.mark.parametrize("batch", [720, 16])
@pytest.mark.parametrize("i,h,launches", SMALL_NETS)
def test_weight_gradient_pair_on_fifteen_tiles(T, i, h, launches, batch):
    rng = np.random.default_rng(SEED + 60 + batch + h)
    ws, X, Y = problem(rng, batch, i, h, 10)
    assert _step_against_the_oracle(T, ws, X, Y) == launches
