"""Where TO_ACT_TANH (3) is accepted by the one-call stack entries and where it is not: hidden_act (and a recurrent layer's
state_act) logistic or tanh; out_act never tanh -- TO_ERR_UNSUPPORTED (5) with nothing written, on every family -- and the
hidden_act values 1 and 7 refused as before."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
LOGISTIC, SOFTMAX, TANH = 0, 2, 3
UNSUPPORTED = 5


@pytest.fixture(scope="module")
def T():
    from tensor_ops_amd.hipt import HipT
    return HipT(0)


def arr(ts):
    from tensor_ops_amd import capi
    return (capi.c_tensor * len(ts))(*[(t.h if t is not None else None) for t in ts])


def test_out_act_tanh_and_unknown_hidden_acts_are_refused(T):
    from tensor_ops_amd import capi
    L = capi.lib()
    rng = np.random.default_rng(41)
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
    # a recurrent stack: one fullyConnected layer, one stateless head
    s, Ws = T.put(rng.standard_normal(14).astype(np.float32)), T.put(rng.standard_normal((14, 14)).astype(np.float32))
    X3, Y3 = T.put(rng.uniform(-1, 1, (B, 4, 30)).astype(np.float32), batched=True), T.put(rng.uniform(0.1, 0.9, (B, 4, 6)).astype(np.float32), batched=True)
    rout = marked((4, 6), B)
    rs, rws, rw, rb = arr([s, None]), arr([Ws, None]), arr(W), arr(b)
    rg = [marked((14,)), marked((14, 14))]
    written = [gW, gB, [losses, out, gx, il, iout, rout], rg]

    def calls(hidden, out_act, loss, sact=(LOGISTIC, -1)):
        sa = (C.c_int * 2)(*sact)
        return {
            "grad": L.to_fflayer_stack_grad(2, arr(W), arr(b), hidden, out_act, loss, x.h, y.h, arr(gW), arr(gB), losses.h),
            "sgd": L.to_fflayer_stack_sgd(2, arr(W), arr(b), hidden, out_act, loss, x.h, y.h, 0.1, losses.h),
            "online": L.to_fflayer_stack_online_sgd(2, arr(W), arr(b), hidden, out_act, loss, x.h, y.h, B, None, 0.1),
            "infer": L.to_fflayer_stack_infer(2, arr(W), arr(b), hidden, out_act, x.h, None, out.h, classes, None),
            "induce": L.to_fflayer_stack_induce(2, arr(W), arr(b), hidden, out_act, loss, x.h, y.h, 0.1, 2, iout.h, gx.h, il.h),
            "rnn_run": L.to_rnn_stack_run(2, sa, rs, rws, rw, rb, hidden, out_act, X3.h, rout.h, None),
            "rnn_grad": L.to_rnn_stack_grad(2, sa, rs, rws, rw, rb, hidden, out_act, loss, X3.h, Y3.h, arr([rg[0], None]),
                                            arr([rg[1], None]), arr(gW), arr(gB), None, None),
            "rnn_sgd": L.to_rnn_stack_sgd(2, sa, rs, rws, rw, rb, hidden, out_act, loss, X3.h, Y3.h, 0.1, 0.1, None),
        }

    def untouched():
        for (w, bb), dw, db in zip(ws, W, b):
            assert np.array_equal(dw.numpy(), w) and np.array_equal(db.numpy(), bb)
        for group in written:
            for t in group:
                assert (t.numpy() == poison).all()
        assert list(classes) == [-5] * B

    for hidden, out_act, loss in ((LOGISTIC, TANH, 1), (LOGISTIC, TANH, 0), (TANH, TANH, 1),   # tanh is no output activation
                                  (1, SOFTMAX, 1), (7, SOFTMAX, 1)):                             # hidden_act 1 and 7: as before
        st = calls(hidden, out_act, loss)
        assert set(st.values()) == {UNSUPPORTED}, (hidden, out_act, loss, st)
        assert b"" != L.to_last_error()
        untouched()
    # a state activation outside {logistic, tanh, stateless}
    sa = (C.c_int * 2)(7, -1)
    assert L.to_rnn_stack_run(2, sa, rs, rws, rw, rb, TANH, SOFTMAX, X3.h, rout.h, None) == UNSUPPORTED
    untouched()
    # ... and tanh where it belongs is taken by every family
    st = calls(TANH, SOFTMAX, 1, sact=(TANH, -1))
    assert set(st.values()) == {0}, (st, L.to_last_error())
