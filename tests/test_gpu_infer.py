"""Batched inference and scoring of ffLayer stacks in one call (to_fflayer_stack_infer, csrc/infer_head.hip):
`runNetwork` (FeedForward.hs:123-129) over a batch with `validate` / `confusion`'s folds (app/MNIST.hs:366-389).

Checked against the oracle's runNetwork row by row, against numpy in fp64 at data-set scale, against to_arg_max of the
rows it stored (bit for bit, ties and NaN included) and np.add.at for the confusion matrix; then the routes' shape edges,
determinism without a clock (a row's bits do not depend on the batch or its place in it) and the call's contract."""
import ctypes as C
import gc

import numpy as np
import pytest

from oracle import neuralnet as NN
from oracle.tensor import OTensor

pytestmark = pytest.mark.gpu
TOL = {np.float32: 1e-5, np.float64: 1e-12}
SOFTMAX, LOGISTIC = 2, 0


@pytest.fixture(scope="module")
def Ts():
    from tensor_ops_amd.hipt import HipT
    return {np.float32: HipT(0, np.float32), np.float64: HipT(0, np.float64)}


def weights(rng, sizes, dt, scale=0.5):
    return [((scale * rng.standard_normal((o, i))).astype(dt), (scale * rng.standard_normal(o)).astype(dt))
            for i, o in zip(sizes[:-1], sizes[1:])]


def forward64(ws, X, head):
    a = X.astype(np.float64)
    for l, (w, b) in enumerate(ws):
        z = a @ w.astype(np.float64).T + b.astype(np.float64)
        if l + 1 < len(ws) or head == "logistic":
            a = 1 / (1 + np.exp(-z))
        else:
            e = np.exp(z - z.max(axis=1, keepdims=True))
            a = e / e.sum(axis=1, keepdims=True)
    return a


def put_net(T, ws):
    return [T.put(w) for w, _ in ws], [T.put(b) for _, b in ws]


def infer(T, ws, bs, x, head="softmax", y=None, want_out=True):
    out, cls, conf = T.infer_stack(ws, bs, x, out_act=head, y=y, want_out=want_out)
    return (out.numpy() if out is not None else None), cls, conf


def onehot(rng, B, n, dt):
    Y = np.zeros((B, n), dt)
    Y[np.arange(B), rng.integers(0, n, B)] = 1
    return Y


@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("head", ["softmax", "logistic"])
@pytest.mark.parametrize("sizes", [[6, 4], [5, 9, 3], [7, 12, 8, 10], [3, 6, 5, 7, 40]])
def test_parity_with_the_oracle(Ts, dt, head, sizes):
    T, O = Ts[dt], OTensor(np.float64)
    rng = np.random.default_rng(len(sizes) * 100 + sizes[-1])
    ws = weights(rng, sizes, dt)
    X = rng.uniform(-1, 1, (64, sizes[0])).astype(dt)
    W, b = put_net(T, ws)
    out, cls, _ = infer(T, W, b, T.put(X, batched=True), head)
    net = NN.genNet([(w.astype(np.float64), bb.astype(np.float64)) for w, bb in ws], NN.actLogistic,
                    NN.actSoftmax if head == "softmax" else NN.actLogistic)
    for r in range(64):
        want = np.asarray(NN.runNetwork(O, net, X[r].astype(np.float64)), np.float64)
        assert np.abs(out[r].astype(np.float64) - want).max() <= TOL[dt], r
    assert np.array_equal(cls, T.arg_max(T.put(out, batched=True)))


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_data_set_scale_784_300_100_10(Ts, dt):
    """60,000 rows of the reference's network; in fp64 the pre-fused path refuses this shape (TO_ERR_UNSUPPORTED)"""
    T = Ts[dt]
    rng = np.random.default_rng(0x1f3)
    ws = weights(rng, [784, 300, 100, 10], dt, scale=0.1)
    X = rng.uniform(0, 1, (60000, 784)).astype(dt)
    Y = onehot(rng, 60000, 10, dt)
    W, b = put_net(T, ws)
    x, y = T.put(X, batched=True), T.put(Y, batched=True)
    out, cls, conf = infer(T, W, b, x, y=y)
    assert np.abs(out - forward64(ws, X, "softmax")).max() <= TOL[dt]
    assert np.array_equal(cls, T.arg_max(T.put(out, batched=True)))
    want = np.zeros((10, 10), np.int64)
    np.add.at(want, (cls, Y.argmax(axis=1)), 1)
    assert np.array_equal(conf, want) and conf.sum() == 60000


@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("nL", [10, 40])
def test_ties_and_nan_follow_to_arg_max(Ts, dt, nL):
    T = Ts[dt]
    rng = np.random.default_rng(nL)
    ws = weights(rng, [13, 9, nL], dt)
    w, bb = ws[-1]
    bb[2] += 4                         # column 2 is the maximum of most rows ...
    w[5], bb[5] = w[2], bb[2]          # ... and so are columns 5 and 7, with equal logits
    w[7], bb[7] = w[2], bb[2]
    X = rng.uniform(-1, 1, (65, 13)).astype(dt)
    X[3, 4] = np.nan                   # a row that is NaN throughout
    for head in ("softmax", "logistic"):
        W, b = put_net(T, ws)
        out, cls, _ = infer(T, W, b, T.put(X, batched=True), head)
        assert np.isnan(out[3]).all()
        assert np.array_equal(cls, T.arg_max(T.put(out, batched=True)))
        finite = np.arange(65) != 3
        assert (cls[finite] == 2).sum() > 30 and not np.isin(cls[finite], [5, 7]).any()   # the earliest of equal maxima
    wn = [(w.copy(), bb.copy()) for w, bb in ws]
    wn[-1][1][1] = np.nan              # logistic head: one NaN column in every row
    W, b = put_net(T, wn)
    out, cls, _ = infer(T, W, b, T.put(X, batched=True), "logistic")
    assert np.isnan(out[:, 1]).all()
    assert np.array_equal(cls, T.arg_max(T.put(out, batched=True)))


@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("nL", [10, 33])
def test_confusion_matrix(Ts, dt, nL):
    T = Ts[dt]
    rng = np.random.default_rng(7 * nL)
    ws = weights(rng, [20, 16, nL], dt)
    X = rng.uniform(-1, 1, (3001, 20)).astype(dt)
    W, b = put_net(T, ws)
    x = T.put(X, batched=True)
    for Y in (onehot(rng, 3001, nL, dt), rng.uniform(0, 1, (3001, nL)).astype(dt)):   # one-hot, then soft targets
        y = T.put(Y, batched=True)
        out, cls, conf = infer(T, W, b, x, y=y)
        actual = Y.argmax(axis=1)
        want = np.zeros((nL, nL), np.int64)
        np.add.at(want, (cls, actual), 1)
        assert np.array_equal(conf, want)
        assert np.trace(conf) == int((cls == actual).sum())
        _, cls2, conf2 = T.infer_stack(W, b, x, y=y, want_classes=False)
        assert cls2 is None and np.array_equal(conf2, conf)


def edge_case(T, dt, nL, K, B, head="softmax", seed=0):
    rng = np.random.default_rng(seed + 1000 * nL + K + B)
    ws = weights(rng, [K, nL], dt, scale=1.0 / np.sqrt(K))
    X = rng.uniform(-1, 1, (B, K)).astype(dt)
    W, b = put_net(T, ws)
    out, cls, conf = infer(T, W, b, T.put(X, batched=True), head)
    assert np.abs(out - forward64(ws, X, head)).max() <= TOL[dt], (nL, K, B)
    assert np.array_equal(cls, T.arg_max(T.put(out, batched=True)))


@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("nL", [1, 2, 10, 16, 17, 31, 32, 33, 64, 1000])
def test_edge_head_widths(Ts, dt, nL):
    for head in ("softmax", "logistic"):
        edge_case(Ts[dt], dt, nL, 100, 65, head)


@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("K", [1, 3, 13, 100, 784, 4097])
def test_edge_fan_in(Ts, dt, K):
    """4097 x 32 does not fit the 64 KiB W_L budget in either dtype: streamed in K chunks"""
    for nL in (10, 32, 33):
        edge_case(Ts[dt], dt, nL, K, 65)


@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("B", [1, 7, 65, 60000])
def test_edge_batch(Ts, dt, B):
    for nL in (10, 64):
        edge_case(Ts[dt], dt, nL, 784, B)


def test_unbatched_x_is_one_row(Ts):
    T = Ts[np.float32]
    rng = np.random.default_rng(3)
    ws = weights(rng, [30, 12, 10], np.float32)
    W, b = put_net(T, ws)
    X = rng.uniform(-1, 1, (1, 30)).astype(np.float32)
    out1, c1, _ = infer(T, W, b, T.put(X[0]))
    outb, cb, _ = infer(T, W, b, T.put(X, batched=True))
    assert out1.shape == (10,) and np.array_equal(out1, outb[0]) and c1.tolist() == cb.tolist()


@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("K", [13, 784])
def test_unaligned_offset_view_is_bitwise_the_aligned_result(Ts, dt, K):
    """x at a one-element offset (the scalar-load path of the narrow head) gives the same bits as the aligned copy (its
    16-byte path at K = 784), for a stack and for a one-layer net whose head reads x itself"""
    from tensor_ops_amd import capi
    from tensor_ops_amd.hipt import DT
    T = Ts[dt]
    rng = np.random.default_rng(K)
    B = 301
    X = rng.uniform(-1, 1, (B, K)).astype(dt)
    buf = T.put(np.concatenate([np.zeros(1, dt), X.ravel()]))
    d = (C.c_int64 * 1)(K)
    h = capi.c_tensor()
    capi.check(capi.lib().to_wrap(C.c_void_p(buf.ptr + np.dtype(dt).itemsize), T.to_dtype, 1, d, B, C.byref(h)))
    xv = DT(h)
    for sizes in ([K, 24, 10], [K, 10], [K, 40]):
        W, b = put_net(T, weights(rng, sizes, dt))
        want, wc, _ = infer(T, W, b, T.put(X, batched=True))
        got, gcl, _ = infer(T, W, b, xv)
        assert np.array_equal(got.view(np.uint8), want.view(np.uint8)) and np.array_equal(gcl, wc), sizes
    del xv


def test_one_layer_narrow_head_is_one_launch(Ts):
    T = Ts[np.float32]
    rng = np.random.default_rng(11)
    ws = weights(rng, [100, 10], np.float32)
    W, b = put_net(T, ws)
    x = T.put(rng.uniform(0, 1, (60000, 100)).astype(np.float32), batched=True)
    infer(T, W, b, x)
    T.sync()
    for want_out in (True, False):
        l0 = T.stats()["launches"]
        T.infer_stack(W, b, x, want_out=want_out)
        assert T.stats()["launches"] - l0 == 1


@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("sizes", [[784, 10], [100, 10], [4097, 32]])
def test_a_row_does_not_depend_on_the_batch(Ts, dt, sizes):
    """the narrow head's order of summation is fixed per row (a stack's hidden layers are GEMMs whose kernel follows
    the batch size); two calls are bitwise identical"""
    T = Ts[dt]
    rng = np.random.default_rng(sizes[-1])
    ws = weights(rng, sizes, dt, scale=0.1)
    X = rng.uniform(0, 1, (60000, sizes[0])).astype(dt)
    r, other = 12345, 59998
    X[other] = X[r]
    X[1998] = X[123]
    W, b = put_net(T, ws)
    x = T.put(X, batched=True)
    out, cls, _ = infer(T, W, b, x)
    out2, cls2, _ = infer(T, W, b, x)
    assert np.array_equal(out.view(np.uint8), out2.view(np.uint8)) and np.array_equal(cls, cls2)
    if sizes[0] > 1000:
        X = X[:2000]
        x = T.put(X, batched=True)
        r, other = 123, 1998
        out, cls, _ = infer(T, W, b, x)
    alone, ca, _ = infer(T, W, b, T.put(X[r:r + 1], batched=True))
    assert np.array_equal(out[r].view(np.uint8), alone[0].view(np.uint8)) and cls[r] == ca[0]
    assert np.array_equal(out[r].view(np.uint8), out[other].view(np.uint8))


def test_contract(Ts):
    from tensor_ops_amd import capi
    from tensor_ops_amd.hipt import Graph
    T = Ts[np.float32]
    rng = np.random.default_rng(99)
    ws = weights(rng, [40, 20, 10], np.float32)
    X, Y = rng.uniform(-1, 1, (500, 40)).astype(np.float32), onehot(rng, 500, 10, np.float32)
    W, b = put_net(T, ws)
    x, y = T.put(X, batched=True), T.put(Y, batched=True)
    gc.collect()
    before = T.stats()["live_handles"]
    out, cls, conf = infer(T, W, b, x, y=y)
    del out
    gc.collect()
    assert T.stats()["live_handles"] == before
    for t, want in zip(W + b + [x, y], [w for w, _ in ws] + [bb for _, bb in ws] + [X, Y]):
        assert np.array_equal(t.numpy().view(np.uint8), want.view(np.uint8))
    # a pending x inside a fusion scope: produced first, same result as the eager value
    want, wc, _ = infer(T, W, b, T.put(2 * X, batched=True))
    with T.memo():
        x2 = T.scaleT(2.0, x)
        got, gcl, _ = infer(T, W, b, x2)
    assert np.array_equal(got, want) and np.array_equal(gcl, wc)
    # refused while a capture records; the capture goes on
    L = capi.lib()
    cls_buf = np.empty(500, np.int64)
    i64 = C.POINTER(C.c_int64)
    from tensor_ops_amd.hipt import _arr
    T.scaleT(3.0, x)
    with Graph() as g:
        st = L.to_fflayer_stack_infer(2, _arr(W), _arr(b), LOGISTIC, SOFTMAX, x.h, None, None,
                                      cls_buf.ctypes.data_as(i64), None)
        h = T.scaleT(3.0, x)
    assert st == 4
    g.launch()
    assert np.array_equal(h.numpy(), 3 * X)

    def status(n=2, Wl=W, bl=b, hidden=LOGISTIC, out_act=SOFTMAX, xx=x, yy=None, oo=None, c=True, m=False):
        cm = np.zeros(100, np.int64)
        return L.to_fflayer_stack_infer(n, _arr(Wl), _arr(bl), hidden, out_act, xx.h, yy.h if yy else None,
                                        oo.h if oo else None, cls_buf.ctypes.data_as(i64) if c else None,
                                        cm.ctypes.data_as(i64) if m else None)
    assert status() == 0
    T64 = Ts[np.float64]
    assert status(xx=T64.put(X.astype(np.float64), batched=True)) == 1          # dtype mix
    assert status(yy=T64.put(Y.astype(np.float64), batched=True), m=True) == 1
    assert status(xx=T.put(X[:, :39], batched=True)) == 2                        # x does not fit W_1
    assert status(Wl=[W[1], W[0]], bl=[b[1], b[0]]) == 2                         # layers do not chain
    assert status(yy=T.put(Y[:, :9], batched=True), m=True) == 2                 # y not n_L wide
    assert status(yy=T.put(Y[:499], batched=True), m=True) == 2                  # y of another batch
    assert status(oo=T.put(np.zeros((500, 9), np.float32), batched=True)) == 2  # out not [B; n_L]
    assert status(m=True) == 1                                                   # confusion without y
    assert status(c=False) == 1                                                  # no output at all
    assert status(n=0) == 1
    assert status(hidden=SOFTMAX) == 5 and status(out_act=7) == 5               # activations outside the contract
