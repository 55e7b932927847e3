"""What the five to_autoencoder_stack_* entries answer to a call with ONE defect: one status from every entry that can see
it, to_last_error() set, every output still holding its poison and every parameter its bits -- and that an sgd refused for
range leaves no parameter half-updated."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
LOGISTIC, SOFTMAX, TANH, IDENTITY = 0, 2, 3, 4
SQUARED_ERROR, CROSS_ENTROPY = 0, 1
OK, ARG, SHAPE, UNSUPPORTED = 0, 1, 2, 5
ALL = ("run", "decode", "grad", "sgd", "minibatch")


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
    rng = np.random.default_rng(53)
    sizes, B = [30, 14, 6, 14, 30], 8
    ws = [(rng.standard_normal((o, i)).astype(np.float32), rng.standard_normal(o).astype(np.float32))
          for i, o in zip(sizes[:-1], sizes[1:])]
    X = rng.uniform(0.1, 0.9, (B, 30)).astype(np.float32)
    W, b = [T.put(w) for w, _ in ws], [T.put(bb) for _, bb in ws]
    x = T.put(X, batched=True)
    poison = np.float32(-77.25)
    marked = lambda shape, batch=0: T.put(np.full(((batch,) if batch else ()) + shape, poison, np.float32), batched=batch > 0)  # noqa: E731
    gW, gB = [marked(w.shape) for w, _ in ws], [marked(bb.shape) for _, bb in ws]
    code, recon, losses, dec = marked((6,), B), marked((30,), B), marked((), B), marked((30,), B)
    code_in = T.put(rng.uniform(0.1, 0.9, (B, 6)).astype(np.float32), batched=True)
    written = [gW, gB, [code, recon, losses, dec]]

    def calls(n_enc=2, n_dec=2, Wl=W, bl=b, xx=x, hidden=LOGISTIC, code_act=TANH, out_act=LOGISTIC, loss=SQUARED_ERROR,
              outs=(code, recon, losses), cin=code_in, dout=dec, only=ALL):
        w_, b_ = arr(Wl), arr(bl)
        h = lambda t: t.h if t is not None else None  # noqa: E731
        entries = {
            "run": lambda: L.to_autoencoder_stack_run(n_enc, n_dec, w_, b_, hidden, code_act, out_act, loss, xx.h, h(outs[0]),
                                                      h(outs[1]), h(outs[2])),
            "decode": lambda: L.to_autoencoder_stack_decode(n_enc, n_dec, w_, b_, hidden, out_act, cin.h, dout.h),
            "grad": lambda: L.to_autoencoder_stack_grad(n_enc, n_dec, w_, b_, hidden, code_act, out_act, loss, xx.h, arr(gW),
                                                        arr(gB), losses.h),
            "sgd": lambda: L.to_autoencoder_stack_sgd(n_enc, n_dec, w_, b_, hidden, code_act, out_act, loss, xx.h, 0.1,
                                                      losses.h),
            "minibatch": lambda: L.to_autoencoder_stack_minibatch_sgd(n_enc, n_dec, w_, b_, hidden, code_act, out_act, loss,
                                                                      xx.h, B, None, 3, 0.1, losses.h),
        }
        st = {}
        for name in only:
            st[name] = entries[name]()
            assert st[name] == OK or L.to_last_error() != b"", name
        return st

    def untouched():
        for (w, bb), dw, db in zip(ws, W, b):
            assert np.array_equal(dw.numpy().view(np.uint32), w.view(np.uint32))
            assert np.array_equal(db.numpy().view(np.uint32), bb.view(np.uint32))
        for group in written:
            for t in group:
                assert (t.numpy() == poison).all()

    T64 = HipT(0, np.float64)
    takes_code = ("run", "grad", "sgd", "minibatch")      # (decode has no code activation and no loss)
    defects = [
        ("code_act = SOFTMAX", dict(code_act=SOFTMAX), UNSUPPORTED, takes_code),
        ("hidden_act = IDENTITY", dict(hidden=IDENTITY), UNSUPPORTED, ALL),
        ("hidden_act = SOFTMAX", dict(hidden=SOFTMAX), UNSUPPORTED, ALL),
        ("(TANH, crossEntropy)", dict(out_act=TANH, loss=CROSS_ENTROPY), UNSUPPORTED, takes_code),
        ("(IDENTITY, crossEntropy)", dict(out_act=IDENTITY, loss=CROSS_ENTROPY), UNSUPPORTED, takes_code),
        ("(LOGISTIC, crossEntropy)", dict(out_act=LOGISTIC, loss=CROSS_ENTROPY), UNSUPPORTED, takes_code),
        ("(SOFTMAX, squaredError)", dict(out_act=SOFTMAX, loss=SQUARED_ERROR), UNSUPPORTED, takes_code),
        ("an output activation nobody knows", dict(out_act=7), UNSUPPORTED, ALL),
        ("n_enc = 0", dict(n_enc=0, n_dec=4), ARG, ALL),
        ("n_dec = 0", dict(n_enc=4, n_dec=0), ARG, ALL),
        ("run with no output asked for", dict(outs=(None, None, None)), ARG, ("run",)),
        ("x in fp64", dict(xx=T64.put(X.astype(np.float64), batched=True)), ARG, takes_code),
        ("the code rows in fp64", dict(cin=T64.put(np.full((B, 6), 0.5), batched=True)), ARG, ("decode",)),
        ("W[3] in fp64", dict(Wl=W[:3] + [T64.put(ws[3][0].astype(np.float64))]), ARG, ALL),
        ("recon in fp64", dict(outs=(code, T64.put(np.full((B, 30), -77.25), batched=True), losses)), ARG, ("run",)),
        ("an output layer of width 29", dict(Wl=W[:3] + [T.put(ws[3][0][:29])], bl=b[:3] + [T.put(ws[3][1][:29])]), SHAPE,
         takes_code),
        ("decode into rows of width 29", dict(dout=marked((29,), B)), SHAPE, ("decode",)),
        ("code of width 5", dict(outs=(marked((5,), B), recon, losses)), SHAPE, ("run",)),
        ("code rows of width 5", dict(cin=T.put(np.full((B, 5), 0.5, np.float32), batched=True)), SHAPE, ("decode",)),
        ("recon of width 29", dict(outs=(code, marked((29,), B), losses)), SHAPE, ("run",)),
        ("losses of another batch", dict(outs=(code, recon, marked((), B + 1))), SHAPE, ("run",)),
    ]
    for what, kw, want, only in defects:
        st = calls(only=only, **kw)
        assert st == {name: want for name in only}, (what, st, L.to_last_error())
        untouched()
        for t in list(kw.get("outs", ())) + [kw.get("dout")]:
            if t is not None and t.numpy().dtype == np.float32:
                assert (t.numpy() == poison).all(), what
    # an output that is an input, another output or a parameter
    both = T.put(np.full((2 * B, 30), poison, np.float32), batched=True)
    for what, kw in (("recon is x", dict(outs=(code, x, losses))),
                     ("recon is the last layer's input rows", dict(outs=(code, recon, losses), xx=recon)),
                     ("recon overlaps recon", dict(outs=(None, T.batch_slice(both, 0, B), None), xx=T.batch_slice(both, B - 1, B)))):
        assert calls(only=("run",), **kw) == {"run": ARG}, what
        untouched()
        assert np.array_equal(x.numpy(), X) and (both.numpy() == poison).all()
    # the existing entries keep refusing tanh as an output activation, and refuse identity anywhere
    for hidden, out_act in ((LOGISTIC, TANH), (LOGISTIC, IDENTITY), (IDENTITY, LOGISTIC)):
        assert L.to_fflayer_stack_grad(4, arr(W), arr(b), hidden, out_act, SQUARED_ERROR, x.h, x.h, arr(gW), arr(gB),
                                       losses.h) == UNSUPPORTED
        assert L.to_fflayer_stack_minibatch_sgd(4, arr(W), arr(b), hidden, out_act, SQUARED_ERROR, x.h, None, B, None, 3, 0.1,
                                                losses.h) == UNSUPPORTED
        assert L.to_fflayer_stack_infer(4, arr(W), arr(b), hidden, out_act, x.h, None, recon.h, None, None) == UNSUPPORTED
        untouched()
    # the well-formed pair is accepted by all five (sgd and minibatch last: they move the parameters)
    st = calls()
    assert set(st.values()) == {OK} and len(st) == 5, (st, L.to_last_error())
    for t in (code, recon, losses, dec, gW[0], gB[-1]):
        assert not (t.numpy() == poison).any()
    assert not np.array_equal(W[0].numpy(), ws[0][0])


def test_run_and_decode_refuse_graph_capture(T):
    from tensor_ops_amd import capi
    from tensor_ops_amd.hipt import Graph
    L = capi.lib()
    rng = np.random.default_rng(59)
    ws = [(rng.standard_normal((o, i)).astype(np.float32), rng.standard_normal(o).astype(np.float32))
          for i, o in zip([8, 3], [3, 8])]
    W, b = [T.put(w) for w, _ in ws], [T.put(bb) for _, bb in ws]
    x = T.put(rng.uniform(0.1, 0.9, (4, 8)).astype(np.float32), batched=True)
    poison = np.float32(-77.25)
    recon = T.put(np.full((4, 8), poison, np.float32), batched=True)
    code = T.put(np.full((4, 3), 0.5, np.float32), batched=True)
    T.scaleT(3.0, x)
    with Graph() as g:                                  # refused while a capture records; the capture goes on
        st = (L.to_autoencoder_stack_run(1, 1, arr(W), arr(b), LOGISTIC, TANH, IDENTITY, SQUARED_ERROR, x.h, None, recon.h, None),
              L.to_autoencoder_stack_decode(1, 1, arr(W), arr(b), LOGISTIC, IDENTITY, code.h, recon.h),
              L.to_autoencoder_stack_minibatch_sgd(1, 1, arr(W), arr(b), LOGISTIC, TANH, IDENTITY, SQUARED_ERROR, x.h, 4, None, 2,
                                                   0.1, None))
        h = T.scaleT(3.0, x)
    g.launch()
    assert st == (4, 4, 4)                               # TO_ERR_STATE
    assert (recon.numpy() == poison).all()
    assert np.array_equal(W[0].numpy(), ws[0][0])


def test_decode_refuses_to_write_over_its_code_rows(T):
    from tensor_ops_amd import capi
    L = capi.lib()
    rng = np.random.default_rng(67)
    ws = [(rng.standard_normal((6, 6)).astype(np.float32), rng.standard_normal(6).astype(np.float32)) for _ in range(2)]
    W, b = [T.put(w) for w, _ in ws], [T.put(bb) for _, bb in ws]
    C0 = rng.uniform(0.1, 0.9, (4, 6)).astype(np.float32)
    c = T.put(C0, batched=True)
    assert L.to_autoencoder_stack_decode(1, 1, arr(W), arr(b), LOGISTIC, TANH, c.h, c.h) == ARG
    assert L.to_last_error() != b"" and np.array_equal(c.numpy(), C0)
    out = T.put(np.zeros((4, 6), np.float32), batched=True)
    assert L.to_autoencoder_stack_decode(1, 1, arr(W), arr(b), LOGISTIC, TANH, c.h, out.h) == OK
    assert np.abs(out.numpy() - np.tanh(C0 @ ws[1][0].T + ws[1][1])).max() <= 1e-5


def test_sgd_refused_for_range_updates_nothing(T):
    """[832, 1024, 832]: the first weight gradient, 1024 x 832, is 16 * 13 = 208 tiles of 64 x 64 -- outside the range of the
    one kernel that applies the update in its epilogue (tests/test_gpu_stack_contract.py).  sgd and minibatch_sgd refuse as
    to_fflayer_stack_sgd does, before they write; grad and run take the same pair."""
    from tensor_ops_amd import capi
    L = capi.lib()
    rng = np.random.default_rng(61)
    sizes, B = [832, 1024, 832], 8
    ws = [((rng.standard_normal((o, i)) / np.sqrt(i)).astype(np.float32), rng.standard_normal(o).astype(np.float32))
          for i, o in zip(sizes[:-1], sizes[1:])]
    W, b = [T.put(w) for w, _ in ws], [T.put(bb) for _, bb in ws]
    x = T.put(rng.uniform(-1, 1, (B, sizes[0])).astype(np.float32), batched=True)
    poison = np.float32(-77.25)
    losses = T.put(np.full((B,), poison, np.float32), batched=True)
    assert L.to_fflayer_stack_sgd(2, arr(W), arr(b), LOGISTIC, LOGISTIC, SQUARED_ERROR, x.h, x.h, 0.1, losses.h) == UNSUPPORTED
    for code_act, out_act in ((LOGISTIC, LOGISTIC), (IDENTITY, TANH)):
        assert L.to_autoencoder_stack_sgd(1, 1, arr(W), arr(b), LOGISTIC, code_act, out_act, SQUARED_ERROR, x.h, 0.1,
                                          losses.h) == UNSUPPORTED
        assert L.to_last_error() != b""
        assert L.to_autoencoder_stack_minibatch_sgd(1, 1, arr(W), arr(b), LOGISTIC, code_act, out_act, SQUARED_ERROR, x.h, B,
                                                    None, 4, 0.1, losses.h) == UNSUPPORTED
        for (w, bb), dw, db in zip(ws, W, b):
            assert np.array_equal(dw.numpy().view(np.uint32), w.view(np.uint32))
            assert np.array_equal(db.numpy().view(np.uint32), bb.view(np.uint32))
        assert (losses.numpy() == poison).all()
    gW, gB = [T.put(np.zeros_like(w)) for w, _ in ws], [T.put(np.zeros_like(bb)) for _, bb in ws]
    assert L.to_autoencoder_stack_grad(1, 1, arr(W), arr(b), LOGISTIC, IDENTITY, TANH, SQUARED_ERROR, x.h, arr(gW), arr(gB),
                                       losses.h) == OK
    assert L.to_autoencoder_stack_run(1, 1, arr(W), arr(b), LOGISTIC, IDENTITY, TANH, SQUARED_ERROR, x.h, None, None,
                                      losses.h) == OK
    assert np.isfinite(losses.numpy()).all() and not (losses.numpy() == poison).any()
