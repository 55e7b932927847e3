"""What the eight one-call stack entries (to_fflayer_stack_grad / _sgd / _online_sgd / _infer / _induce, to_rnn_stack_run /
_grad / _sgd) answer to a stack with ONE defect: the same status from every entry, to_last_error() set, nothing written --
and that a refused to_fflayer_stack_sgd leaves no parameter half-updated."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
LOGISTIC, SOFTMAX = 0, 2
SQUARED_ERROR, CROSS_ENTROPY = 0, 1
OK, ARG, SHAPE, UNSUPPORTED = 0, 1, 2, 5
TAKES_LOSS = ("grad", "sgd", "online", "induce", "rnn_grad", "rnn_sgd")


@pytest.fixture(scope="module")
def T():
    from tensor_ops_amd.hipt import HipT
    return HipT(0)


def arr(ts):
    from tensor_ops_amd import capi
    return (capi.c_tensor * len(ts))(*[(t.h if t is not None else None) for t in ts])


def test_one_defect_one_status_nothing_written(T):
    from tensor_ops_amd import capi
    from tensor_ops_amd.hipt import HipT
    L = capi.lib()
    rng = np.random.default_rng(43)
    sizes, B = [30, 14, 6], 8
    ws = [(rng.standard_normal((o, i)).astype(np.float32), rng.standard_normal(o).astype(np.float32))
          for i, o in zip(sizes[:-1], sizes[1:])]
    X = rng.uniform(-1, 1, (B, 30)).astype(np.float32)
    Y = rng.uniform(0.1, 0.9, (B, 6)).astype(np.float32)
    W, b = [T.put(w) for w, _ in ws], [T.put(bb) for _, bb in ws]
    x, y = T.put(X, batched=True), T.put(Y, batched=True)
    poison = np.float32(-77.25)
    marked = lambda shape, batch=0: T.put(np.full(((batch,) if batch else ()) + shape, poison, np.float32), batched=batch > 0)  # noqa: E731
    gW, gB = [marked(w.shape) for w, _ in ws], [marked(bb.shape) for _, bb in ws]
    losses, out, gx, il, iout = marked((), B), marked((6,), B), marked((30,), B), marked((2,), B), marked((30,), B)
    classes = (C.c_int64 * B)(*([-5] * B))
    # the recurrent twin: one fullyConnected layer, one stateless head, T = 4
    s, Ws = T.put(rng.standard_normal(14).astype(np.float32)), T.put(rng.standard_normal((14, 14)).astype(np.float32))
    X3, Y3 = T.put(rng.uniform(-1, 1, (B, 4, 30)).astype(np.float32), batched=True), T.put(rng.uniform(0.1, 0.9, (B, 4, 6)).astype(np.float32), batched=True)
    rout = marked((4, 6), B)
    rs, rws = arr([s, None]), arr([Ws, None])
    rg = [marked((14,)), marked((14, 14))]
    written = [gW, gB, [losses, out, gx, il, iout, rout], rg]
    sa = (C.c_int * 2)(LOGISTIC, -1)

    def calls(n=2, Wl=W, bl=b, yy=y, YY=Y3, out_act=SOFTMAX, loss=CROSS_ENTROPY, only=None):
        w_, b_ = arr(Wl), arr(bl)
        entries = {
            "grad": lambda: L.to_fflayer_stack_grad(n, w_, b_, LOGISTIC, out_act, loss, x.h, yy.h, arr(gW), arr(gB), losses.h),
            "sgd": lambda: L.to_fflayer_stack_sgd(n, w_, b_, LOGISTIC, out_act, loss, x.h, yy.h, 0.1, losses.h),
            "online": lambda: L.to_fflayer_stack_online_sgd(n, w_, b_, LOGISTIC, out_act, loss, x.h, yy.h, B, None, 0.1),
            "infer": lambda: L.to_fflayer_stack_infer(n, w_, b_, LOGISTIC, out_act, x.h, yy.h, out.h, classes, None),
            "induce": lambda: L.to_fflayer_stack_induce(n, w_, b_, LOGISTIC, out_act, loss, x.h, yy.h, 0.1, 2, iout.h, gx.h, il.h),
            "rnn_run": lambda: L.to_rnn_stack_run(n, sa, rs, rws, w_, b_, LOGISTIC, out_act, X3.h, rout.h, None),
            "rnn_grad": lambda: L.to_rnn_stack_grad(n, sa, rs, rws, w_, b_, LOGISTIC, out_act, loss, X3.h, YY.h, arr([rg[0], None]),
                                                    arr([rg[1], None]), arr(gW), arr(gB), None, None),
            "rnn_sgd": lambda: L.to_rnn_stack_sgd(n, sa, rs, rws, w_, b_, LOGISTIC, out_act, loss, X3.h, YY.h, 0.1, 0.1, None),
        }
        st = {}
        for name, f in entries.items():
            if only is None or name in only:
                st[name] = f()
                assert st[name] == OK or L.to_last_error() != b"", name
        return st

    def untouched():
        for (w, bb), dw, db in zip(ws, W, b):
            assert np.array_equal(dw.numpy(), w) and np.array_equal(db.numpy(), bb)
        for group in written:
            for t in group:
                assert (t.numpy() == poison).all()
        assert list(classes) == [-5] * B

    T64 = HipT(0, np.float64)
    defects = [
        ("W[1] of shape [6, 13]", dict(Wl=[W[0], T.put(ws[1][0][:, :13])]), SHAPE, None),
        ("b[0] of length 13", dict(bl=[T.put(ws[0][1][:13]), b[1]]), SHAPE, None),
        ("W[0] in fp64", dict(Wl=[T64.put(ws[0][0].astype(np.float64)), W[1]]), ARG, None),
        ("a null w[1]", dict(Wl=[W[0], None]), ARG, None),
        ("n_layers = 0", dict(n=0), ARG, None),
        ("targets of width 5", dict(yy=T.put(Y[:, :5], batched=True), YY=T.put(np.full((B, 4, 5), 0.5, np.float32), batched=True)),
         SHAPE, TAKES_LOSS + ("infer",)),
        ("(softmax, squaredError)", dict(loss=SQUARED_ERROR), UNSUPPORTED, TAKES_LOSS),
    ]
    for what, kw, want, only in defects:
        st = calls(only=only, **kw)
        expect = {name: want for name in st}
        if what == "n_layers = 0":
            expect["online"] = UNSUPPORTED   # its own rule: 2..6 layers
        assert st == expect, (what, st)
        untouched()
    # an entry without a loss does not look at one
    assert calls(loss=SQUARED_ERROR, only=("infer", "rnn_run")) == {"infer": OK, "rnn_run": OK}
    # the well-formed stack is accepted by all eight
    st = calls()
    assert set(st.values()) == {OK} and len(st) == 8, (st, L.to_last_error())


def test_refused_sgd_updates_nothing(T):
    """[832, 1024, 6]: the first weight gradient, 1024 x 832, is 16 * 13 = 208 tiles of 64 x 64 -- outside the range of the one
    kernel that applies the update in its epilogue.  sgd refuses before it writes; grad takes the same stack."""
    from tensor_ops_amd import capi
    L = capi.lib()
    rng = np.random.default_rng(47)
    sizes, B = [832, 1024, 6], 8
    ws = [((rng.standard_normal((o, i)) / np.sqrt(i)).astype(np.float32), rng.standard_normal(o).astype(np.float32))
          for i, o in zip(sizes[:-1], sizes[1:])]
    W, b = [T.put(w) for w, _ in ws], [T.put(bb) for _, bb in ws]
    x = T.put(rng.uniform(-1, 1, (B, sizes[0])).astype(np.float32), batched=True)
    y = T.put(rng.uniform(0.1, 0.9, (B, sizes[-1])).astype(np.float32), batched=True)
    assert L.to_fflayer_stack_sgd(2, arr(W), arr(b), LOGISTIC, SOFTMAX, CROSS_ENTROPY, x.h, y.h, 0.1, None) == UNSUPPORTED
    assert L.to_last_error() != b""
    for (w, bb), dw, db in zip(ws, W, b):
        assert np.array_equal(dw.numpy().view(np.uint32), w.view(np.uint32))
        assert np.array_equal(db.numpy().view(np.uint32), bb.view(np.uint32))
    gW, gB = [T.put(np.zeros_like(w)) for w, _ in ws], [T.put(np.zeros_like(bb)) for _, bb in ws]
    assert L.to_fflayer_stack_grad(2, arr(W), arr(b), LOGISTIC, SOFTMAX, CROSS_ENTROPY, x.h, y.h, arr(gW), arr(gB), None) == OK
