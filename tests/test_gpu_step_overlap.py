"""The two GEMM-shaped launches of the batched step after their load / MFMA schedules were rearranged:

* the forward kernel (gemm_t32.hip) runs EIGHT waves a tile wherever the tile grid is at most one round of the device's
  CUs -- K split eight ways in units of 16, one chunk in flight per wave, the eight partial tiles added in wave order --
  and keeps four waves above that;
* the weight-gradient pair (gemm_small.hip) issues each wave's K slice in parts, pinned against its MFMAs.  The K
  partition over the waves and the order in which the sixteen partials are added did not change.

Small-integer operands make every product and every partial sum exact in fp32 whatever the summation order, so the
eight-wave form is compared bit for bit; the pair runs on random fp32 data against the fp64 oracle at the project's 1e-5
(reproducing the MFMA's internal order of additions on the host is not cheap; bit-identity with the parent commit was
established once on dumped outputs, profiles/README.md)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = 0x7e500051
RTOL = 1e-5


@pytest.fixture(scope="module")
def T():
    from tensor_ops_amd.hipt import HipT
    return HipT(0)


def _flat_grads(tr):
    import ctypes as C
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


# (M, K, N): the step's forward shape (256 tiles, K = 49 units of 16: seven waves take 6 and one 7); K = 788 (50 units:
# 6, 6, 6, 7, 6, 6, 6, 7, and a last chunk of 4 k) and K = 272 (17 units: 2, 2, 2, 2, 2, 2, 2, 3 -- runs of one chunk);
# edge tiles in both extents; and two shapes ABOVE one round of 256 CUs (512 and 272 tiles), which keep four waves
SHAPES = [(1024, 784, 256), (1024, 788, 256), (1024, 272, 256), (992, 788, 252), (1024, 784, 512), (1088, 784, 256)]


@pytest.mark.parametrize("ta,tb", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("m,k,n", SHAPES)
def test_forward_tiles_bit_exact_on_integers_in_every_layout(T, m, k, n, ta, tb):
    rng = np.random.default_rng(SEED + 2 * ta + tb)
    a = rng.integers(-2, 3, size=(m, k)).astype(np.float32)
    b = rng.integers(-2, 3, size=(k, n)).astype(np.float32)
    da = T.transp(T.put(np.ascontiguousarray(a.T))) if ta else T.put(a)
    db = T.transp(T.put(np.ascontiguousarray(b.T))) if tb else T.put(b)
    got = T.gmul(1, 1, 1, da, db).numpy()
    want = (a.astype(np.float64) @ b.astype(np.float64)).astype(np.float32)
    assert np.array_equal(got, want), (int(np.sum(got != want)), np.argwhere(got != want)[:4].tolist())


@pytest.mark.parametrize("rows,i,o", [(1024, 784, 256), (992, 788, 252), (1024, 272, 256)])
def test_forward_layer_with_bias_and_logistic_in_the_epilogue(T, rows, i, o):
    """`W x + b` exact on integers, and under the logistic at the 2e-6 absolute bound of tools/t32_check.py"""
    from tensor_ops_amd import hipt
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
        h = T.force(T.liftT(hipt.logistic_closure, [T.sumT([T.matVec(dW, dX), db], (o,))], key="overlap-logistic"))
    err = np.max(np.abs(h.numpy().reshape(rows, o) - 1 / (1 + np.exp(-want))))
    print("max abs error under the logistic:", err)
    assert err < 2e-6


@pytest.mark.parametrize("batch", [1024, 1000])
def test_weight_gradient_pair_on_random_data(T, batch):
    """the step's own shapes (K = the batch = 1024) and a ragged pair (K = 1000: the last wave's slice is short, its loads
    beyond K return zeros through the buffer descriptor): gradients and the updated parameters against the fp64 oracle"""
    import bench
    from oracle import hmat
    from tensor_ops_amd import tops
    ws, X, Y = bench.synth(3, batch)
    want, _ = hmat.batched_grads(X, Y, ws[0][0], ws[0][1], ws[1][0], ws[1][1], recompute=False)
    net = tops.genNet([(T.put(w), T.put(b)) for w, b in ws], "actMapLogistic", "actSoftmax")
    tr = tops.Trainer(net, "crossEntropy", 0.02, T.put(X, batched=True), T.put(Y, batched=True))
    tr.grad()
    assert tr.launches_per_step == 3   # forward; loss head + dZ1; the weight-gradient pair
    for name, g, w in zip(("dW1", "db1", "dW2", "db2"), _split(_flat_grads(tr), [(256, 784), (256,), (10, 256), (10,)]), want):
        e = rel_err(g, w)
        print(name, "rel_err", e)
        assert e < RTOL
    tr.apply()
    for name, p, w0, g in zip(("W1", "b1", "W2", "b2"), tr.net.params, [ws[0][0], ws[0][1], ws[1][0], ws[1][1]], want):
        e = rel_err(p.numpy(), w0 - 0.02 * g)
        print(name, "updated, rel_err", e)
        assert e < RTOL
