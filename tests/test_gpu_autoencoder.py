"""to_autoencoder_stack_run / _decode / _grad / _sgd / _minibatch_sgd: AutoEncoder.hs in one call.

The reference for values is tests/autoencoder_numpy.py in float64 (held to oracle/autoencoder.py by
tests/test_autoencoder_numpy_ref.py) on the parameters and rows as stored in the element type under test; the tolerances
are those of tests/test_gpu_stack_tanh.py: relative 1e-5 / 1e-11 for grad and sgd, absolute 1e-5 / 1e-12 for run and decode.
A per-row loss in the absolute regime is measured as that file's test_induce measures one -- the difference over
max(1, largest loss) -- because a sum over a thousand elements lies above 1, where one ulp of fp32 already exceeds 1e-5.

Shapes.  The head kernel (csrc/recon_head.hip) holds a row tile of 1,024 elements in registers in 16-byte pieces: widths 1, 3
(less than a piece), 64, 65 (fp32 / fp64 rows that are no whole number of pieces: the element path), 68 (whole pieces, a
partly filled tile), 1024 (one full tile), 1028 (a second tile, whole pieces) and 1031 (a second tile on the element path);
one row and five rows (a partly filled workgroup of four waves, and a second workgroup); rows that start at row 1 of a
larger tensor have an unaligned base.  The steps: [30, 14, 6, 14, 30] has a head wider than 16 (no fused head for the old
pairs), [12, 8, 5, 12] and [12, 5, 12] reach the old pairs' fused head and tail with the code layer right below it,
[20, 8, 12, 16, 20] has a one-layer encoder, B = 1 is the rank-1 route and [784, 256, 784] at 1,024 rows the reference's
width on the big GEMM routes."""
import itertools

import numpy as np
import pytest

import autoencoder_numpy as AEN

pytestmark = pytest.mark.gpu
DTS = [np.float32, np.float64]
RTOL = {np.float32: 1e-5, np.float64: 1e-11}      # tests/test_gpu_stack_tanh.py: grad / sgd
ATOL = {np.float32: 1e-5, np.float64: 1e-12}      # tests/test_gpu_stack_tanh.py: infer / induce
PAIRS = list(AEN.PAIRS.items())                   # (out_act, loss)
OLD = ["softmax", "logistic"]                     # the out_acts of to_fflayer_stack_*'s two pairs
OK, UNSUPPORTED = 0, 5


@pytest.fixture(scope="module")
def Ts():
    from tensor_ops_amd.hipt import HipT
    return {np.float32: HipT(0, np.float32), np.float64: HipT(0, np.float64)}


def ident(v):
    if isinstance(v, list):
        return "-".join(map(str, v))
    return getattr(v, "__name__", str(v))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def rel_err(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    return np.linalg.norm((got - want).ravel()) / max(np.linalg.norm(want.ravel()), 1e-300)


def abs_err(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    return np.abs(got - want).max()


def loss_err(got, want):
    return abs_err(got, want) / max(1.0, np.abs(want).max())


def rows_for(out_act, rng, B, n, dt):
    """rows in the range of the head's activation; for softmax normalised to sum 1"""
    X = rng.uniform(0.05, 0.95, (B, n))
    if out_act == "softmax":
        X = X / X.sum(axis=1, keepdims=True)
    elif out_act != "logistic":
        X = 2 * X - 1
    return X.astype(dt)


def problem(sizes, B, dt, seed, out_act):
    """weights N(0, 1 / fan_in)"""
    rng = np.random.default_rng(seed)
    ws = [((rng.standard_normal((o, i)) / np.sqrt(i)).astype(dt), (0.5 * rng.standard_normal(o)).astype(dt))
          for i, o in zip(sizes[:-1], sizes[1:])]
    return ws, rows_for(out_act, rng, B, sizes[0], dt)


def put_net(T, ws):
    return [T.put(w) for w, _ in ws], [T.put(b) for _, b in ws]


def params(W, b):
    return [t.numpy() for t in W] + [t.numpy() for t in b]


# ---- 1. the head kernel through run, all three outputs ----------------------------------------------------------------------
def check_run(T, dt, ws, n_enc, x, X, hidden, code_act, out_act):
    W, b = put_net(T, ws)
    code, recon, losses = T.autoencoder_run(W, b, n_enc, x, out_act, AEN.PAIRS[out_act], hidden, code_act)
    wc, wr, wl = AEN.run(ws, n_enc, X, hidden, code_act, out_act)
    errs = (abs_err(code.numpy(), wc), abs_err(recon.numpy(), wr), loss_err(losses.numpy(), wl))
    print("run", dt.__name__, [w.shape[0] for w, _ in ws], X.shape, hidden, code_act, out_act, errs)
    assert max(errs) <= ATOL[dt]
    return code, recon, losses, W, b


@pytest.mark.parametrize("dt", DTS, ids=ident)
@pytest.mark.parametrize("n", [1, 3, 64, 65, 68, 1024, 1028, 1031])
def test_head_through_run(Ts, n, dt):
    T = Ts[dt]
    for B, (out_act, _) in itertools.product((1, 5), PAIRS):
        ws, X = problem([n, 5, n], B, dt, 0xae0 + n + B, out_act)
        check_run(T, dt, ws, 1, T.put(X, batched=True), X, "logistic", "tanh", out_act)
    # one unbatched row
    ws, X = problem([n, 5, n], 1, dt, 0xae1 + n, "tanh")
    check_run(T, dt, ws, 1, T.put(X[0]), X[0], "tanh", "identity", "tanh")


@pytest.mark.parametrize("dt", DTS, ids=ident)
@pytest.mark.parametrize("n", [3, 65])
def test_head_on_rows_with_an_unaligned_base(Ts, n, dt):
    T = Ts[dt]
    for B, (out_act, _) in itertools.product((1, 5), PAIRS):
        ws, X = problem([n, 5, n], B + 2, dt, 0xae2 + n + B, out_act)
        full = T.put(X, batched=True)
        x = T.batch_slice(full, 1, B)
        assert x.ptr % 16 != 0
        check_run(T, dt, ws, 1, x, X[1:1 + B], "logistic", "tanh", out_act)
        assert same_bits(full.numpy(), X)


# ---- 2. run's outputs ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS, ids=ident)
@pytest.mark.parametrize("sizes,n_enc", [([30, 14, 6, 14, 30], 2), ([1031, 5, 1031], 1)], ids=ident)
def test_run_outputs_do_not_depend_on_each_other(Ts, sizes, n_enc, dt):
    T = Ts[dt]
    for out_act, loss in PAIRS:
        ws, X = problem(sizes, 7, dt, 0xae3 + len(sizes), out_act)
        x = T.put(X, batched=True)
        code, recon, losses, W, b = check_run(T, dt, ws, n_enc, x, X, "tanh", "identity", out_act)
        kw = dict(out_act=out_act, loss=loss, hidden_act="tanh", code_act="identity")
        n0 = T.stats()["launches"]
        c1, r1, l1 = T.autoencoder_run(W, b, n_enc, x, want_code=False, want_recon=False, **kw)
        k_loss = T.stats()["launches"] - n0
        assert c1 is None and r1 is None and same_bits(l1.numpy(), losses.numpy())
        c2, r2, l2 = T.autoencoder_run(W, b, n_enc, x, want_code=False, want_losses=False, **kw)
        assert same_bits(r2.numpy(), recon.numpy()) and l2 is None
        n0 = T.stats()["launches"]
        c3, r3, l3 = T.autoencoder_run(W, b, n_enc, x, want_recon=False, want_losses=False, **kw)
        k_code = T.stats()["launches"] - n0
        assert same_bits(c3.numpy(), code.numpy()) and r3 is None and l3 is None
        assert k_code < k_loss                      # code alone: the decoder is not run
        dec = T.autoencoder_decode(W, b, n_enc, code, out_act, "tanh")
        err = abs_err(dec.numpy(), recon.numpy())
        print("decode", dt.__name__, sizes, out_act, err)
        assert err <= ATOL[dt]
        assert abs_err(dec.numpy(), AEN.decode(ws, n_enc, code.numpy(), "tanh", out_act)) <= ATOL[dt]
        assert same_bits(x.numpy(), X) and all(same_bits(p, q) for p, q in zip(params(W, b), [w for w, _ in ws] + [bb for _, bb in ws]))


# ---- 3. grad then sgd, against numpy ---------------------------------------------------------------------------------------
def check_step(T, dt, sizes, n_enc, B, hidden, code_act, out_act, seed):
    loss = AEN.PAIRS[out_act]
    ws, X = problem(sizes, B, dt, seed, out_act)
    want_g, want_l, _ = AEN.grads(ws, n_enc, X, hidden, code_act, out_act)
    W, b = put_net(T, ws)
    x = T.put(X, batched=True)
    gW, gB, losses = T.autoencoder_grad(W, b, n_enc, x, out_act, loss, hidden, code_act, want_losses=True)
    errs = [rel_err(g.numpy(), w) for g, (w, _) in zip(gW, want_g)] + [rel_err(g.numpy(), w) for g, (_, w) in zip(gB, want_g)]
    lerr = rel_err(losses.numpy(), want_l)
    print("grad", dt.__name__, sizes, n_enc, B, hidden, code_act, out_act, errs, "losses", lerr)
    assert max(errs) < RTOL[dt] and lerr < RTOL[dt]
    for (w, bb), dw, db in zip(ws, W, b):       # the gradients' call leaves the parameters alone
        assert same_bits(dw.numpy(), w) and same_bits(db.numpy(), bb)
    rate = 0.05
    l2 = T.autoencoder_sgd(W, b, n_enc, x, rate, out_act, loss, hidden, code_act, want_losses=True)
    want = AEN.sgd(ws, n_enc, X, rate, hidden, code_act, out_act)
    errs = [max(rel_err(dw.numpy(), w), rel_err(db.numpy(), bb)) for (w, bb), dw, db in zip(want, W, b)]
    print("sgd", errs)
    assert max(errs) < RTOL[dt] and same_bits(l2.numpy(), losses.numpy())
    assert not np.array_equal(W[0].numpy(), ws[0][0])   # ... and the step moved them
    assert same_bits(x.numpy(), X)


@pytest.mark.parametrize("dt", DTS, ids=ident)
@pytest.mark.parametrize("out_act", list(AEN.PAIRS))
@pytest.mark.parametrize("code_act", AEN.CODE)
@pytest.mark.parametrize("hidden", AEN.HIDDEN)
def test_grad_and_sgd_every_combination(Ts, hidden, code_act, out_act, dt):
    check_step(Ts[dt], dt, [30, 14, 6, 14, 30], 2, 64, hidden, code_act, out_act, 0xae4)


# (sizes, n_enc, B, hidden, code_act)
STEPS = [
    ([12, 8, 5, 12], 2, 64, "logistic", "tanh"),        # the old pairs' fused head and tail, the code layer right below
    ([12, 8, 5, 12], 2, 64, "logistic", "identity"),    # ... and no tail behind an identity
    ([12, 5, 12], 1, 64, "logistic", "tanh"),
    ([12, 5, 12], 1, 64, "logistic", "identity"),
    ([20, 8, 12, 16, 20], 1, 64, "tanh", "identity"),   # a one-layer encoder
    ([20, 8, 12, 16, 20], 1, 64, "logistic", "tanh"),
    ([30, 14, 6, 14, 30], 2, 1, "tanh", "identity"),    # one sample: the rank-1 route
    ([12, 5, 12], 1, 1, "logistic", "tanh"),
]


@pytest.mark.parametrize("dt", DTS, ids=ident)
@pytest.mark.parametrize("sizes,n_enc,B,hidden,code_act", STEPS, ids=ident)
def test_grad_and_sgd_routes(Ts, sizes, n_enc, B, hidden, code_act, dt):
    for out_act in AEN.PAIRS:
        check_step(Ts[dt], dt, sizes, n_enc, B, hidden, code_act, out_act, 0xae5 + B + len(sizes))


@pytest.mark.parametrize("hidden,code_act,out_act", [("logistic", "logistic", "logistic"), ("tanh", "identity", "identity"),
                                                     ("logistic", "tanh", "tanh"), ("tanh", "tanh", "softmax")])
def test_the_reference_width_answers_like_the_existing_entry(Ts, hidden, code_act, out_act):
    """[784, 256, 784] at 1,024 rows in fp32: whatever to_fflayer_stack_sgd answers to this shape with y = x, the new entry
    answers; where that is success, its values are compared."""
    dt = np.float32
    T = Ts[dt]
    sizes, B = [784, 256, 784], 1024
    ws, X = problem(sizes, B, dt, 0xae6, "logistic")
    W, b = put_net(T, ws)
    x = T.put(X, batched=True)
    from tensor_ops_amd import capi
    from tensor_ops_amd.hipt import _arr
    old = capi.lib().to_fflayer_stack_sgd(2, _arr(W), _arr(b), 0, 0, 0, x.h, x.h, 0.01, None)
    assert old in (OK, UNSUPPORTED)
    ws, X = problem(sizes, B, dt, 0xae6, out_act)
    W, b = put_net(T, ws)
    x = T.put(X, batched=True)
    args = T._ae_args(W, b, 1, hidden, code_act, out_act, AEN.PAIRS[out_act])
    new = capi.lib().to_autoencoder_stack_sgd(*args, x.h, 0.01, None)
    assert new == old
    if new == OK:
        want = AEN.sgd(ws, 1, X, 0.01, hidden, code_act, out_act)
        errs = [max(rel_err(dw.numpy(), w), rel_err(db.numpy(), bb)) for (w, bb), dw, db in zip(want, W, b)]
        print("sgd 784-256-784", hidden, code_act, out_act, errs)
        assert max(errs) < RTOL[dt]
        assert not np.array_equal(W[0].numpy(), ws[0][0])
    else:
        assert all(same_bits(p, q) for p, q in zip(params(W, b), [w for w, _ in ws] + [bb for _, bb in ws]))


# ---- 4. uniform stacks with the old pairs: to_fflayer_stack_*'s launches and bits ----------------------------------------
def counted(T, f):
    n0 = T.stats()["launches"]
    r = f()
    return r, T.stats()["launches"] - n0


@pytest.mark.parametrize("dt", DTS, ids=ident)
@pytest.mark.parametrize("sizes,n_enc,B", [([30, 14, 6, 14, 30], 2, 64), ([12, 8, 5, 12], 2, 64), ([12, 5, 12], 1, 64),
                                           ([12, 5, 12], 1, 1)], ids=ident)
def test_uniform_stack_is_the_fflayer_entry_bit_for_bit(Ts, sizes, n_enc, B, dt):
    T = Ts[dt]
    for hidden, out_act in itertools.product(AEN.HIDDEN, OLD):
        loss = AEN.PAIRS[out_act]
        ws, X = problem(sizes, B, dt, 0xae7 + B, out_act)
        x = T.put(X, batched=True)
        W1, b1 = put_net(T, ws)
        (g1w, g1b, l1), k1 = counted(T, lambda: T.stack_grad(W1, b1, x, x, out_act, loss, hidden_act=hidden, want_losses=True))
        W2, b2 = put_net(T, ws)
        (g2w, g2b, l2), k2 = counted(T, lambda: T.autoencoder_grad(W2, b2, n_enc, x, out_act, loss, hidden, hidden, want_losses=True))
        assert k1 == k2 and same_bits(l1.numpy(), l2.numpy())
        assert all(same_bits(p.numpy(), q.numpy()) for p, q in zip(g1w + g1b, g2w + g2b))
        s1, k1 = counted(T, lambda: T.stack_sgd(W1, b1, x, x, 0.05, out_act, loss, hidden_act=hidden, want_losses=True))
        s2, k2 = counted(T, lambda: T.autoencoder_sgd(W2, b2, n_enc, x, 0.05, out_act, loss, hidden, hidden, want_losses=True))
        assert k1 == k2 and same_bits(s1.numpy(), s2.numpy())
        assert all(same_bits(p, q) for p, q in zip(params(W1, b1), params(W2, b2)))
        assert not np.array_equal(W2[0].numpy(), ws[0][0])
        # a code activation that is the other of logistic / tanh: the launch count of the uniform stack
        other = "tanh" if hidden == "logistic" else "logistic"
        W3, b3 = put_net(T, ws)
        _, k3 = counted(T, lambda: T.autoencoder_sgd(W3, b3, n_enc, x, 0.05, out_act, loss, hidden, other))
        assert k3 == k2


@pytest.mark.parametrize("dt", DTS, ids=ident)
@pytest.mark.parametrize("out_act", OLD)
def test_uniform_minibatch_is_the_fflayer_entry_bit_for_bit(Ts, out_act, dt):
    T = Ts[dt]
    sizes, n_enc, N, M = [30, 14, 6, 14, 30], 2, 50, 16
    loss = AEN.PAIRS[out_act]
    ws, X = problem(sizes, N, dt, 0xae8, out_act)
    x = T.put(X, batched=True)
    idx = np.random.default_rng(5).integers(0, N, 40).astype(np.int64)     # 16 + 16 + a tail of 8, with repeats
    idx[17] = idx[16]
    for ix, n in ((idx, None), (None, 40), (None, None)):
        W1, b1 = put_net(T, ws)
        l1, k1 = counted(T, lambda: T.stack_minibatch_sgd(W1, b1, x, None, 0.05, M, idx=ix, n=n, out_act=out_act, loss=loss,
                                                          hidden_act="tanh", want_losses=True))
        W2, b2 = put_net(T, ws)
        l2, k2 = counted(T, lambda: T.autoencoder_minibatch_sgd(W2, b2, n_enc, x, 0.05, M, idx=ix, n=n, out_act=out_act,
                                                                loss=loss, hidden_act="tanh", code_act="tanh",
                                                                want_losses=True))
        assert k1 == k2 and same_bits(l1.numpy(), l2.numpy())
        assert all(same_bits(p, q) for p, q in zip(params(W1, b1), params(W2, b2)))
        assert not np.array_equal(W2[0].numpy(), ws[0][0])
    assert same_bits(x.numpy(), X)


# ---- 5. minibatch_sgd for a new pair ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS, ids=ident)
def test_minibatch_sgd_is_the_host_loop_of_sgd(Ts, dt):
    """[30, 14, 30], tanh with squaredError, N = 50, minibatch 16 with a tail, repeated indices: parameters and losses are
    those of to_autoencoder_stack_sgd on the gathered rows, step by step, bit for bit."""
    T = Ts[dt]
    sizes, N, M = [30, 14, 30], 50, 16
    ws, X = problem(sizes, N, dt, 0xae9, "tanh")
    x = T.put(X, batched=True)
    idx = np.random.default_rng(6).integers(0, N, 40).astype(np.int64)
    idx[0], idx[-1], idx[17] = 0, N - 1, idx[16]
    kw = dict(out_act="tanh", loss="squaredError", hidden_act="logistic", code_act="identity")
    W1, b1 = put_net(T, ws)
    want = []
    for s in range(0, len(idx), M):
        want.append(T.autoencoder_sgd(W1, b1, 1, T.batch_gather(x, idx[s:s + M]), 0.05, want_losses=True, **kw).numpy())
    W2, b2 = put_net(T, ws)
    got = T.autoencoder_minibatch_sgd(W2, b2, 1, x, 0.05, M, idx=idx, want_losses=True, **kw)
    assert same_bits(got.numpy(), np.concatenate(want))
    assert all(same_bits(p, q) for p, q in zip(params(W1, b1), params(W2, b2)))
    assert not np.array_equal(W2[0].numpy(), ws[0][0])
    # ... and against numpy
    cur = ws
    for s in range(0, len(idx), M):
        cur = AEN.sgd(cur, 1, X[idx[s:s + M]], 0.05, "logistic", "identity", "tanh")
    errs = [max(rel_err(dw.numpy(), w), rel_err(db.numpy(), bb)) for (w, bb), dw, db in zip(cur, W2, b2)]
    print("minibatch", dt.__name__, errs)
    assert max(errs) < RTOL[dt]
    assert same_bits(x.numpy(), X)


# ---- 6. saturation -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS, ids=ident)
@pytest.mark.parametrize("out_act", ["logistic", "tanh"])
def test_saturated_heads_stay_finite(Ts, out_act, dt):
    """last-layer biases of +-200: exp overflows in fp32, the activation is 0 / 1 / -1 to the last bit, dz is finite (0 where
    act' vanishes) and the losses match numpy"""
    T = Ts[dt]
    sizes, B = [30, 14, 30], 8
    ws, X = problem(sizes, B, dt, 0xaea, out_act)
    sat = np.where(np.arange(30) % 2 == 0, 200.0, -200.0).astype(dt)
    ws[-1] = (ws[-1][0], sat)
    W, b = put_net(T, ws)
    x = T.put(X, batched=True)
    gW, gB, losses = T.autoencoder_grad(W, b, 1, x, out_act, "squaredError", "logistic", "tanh", want_losses=True)
    want_g, want_l, _ = AEN.grads(ws, 1, X, "logistic", "tanh", out_act)
    got = [g.numpy() for g in gW + gB]
    assert all(np.isfinite(g).all() for g in got) and np.isfinite(losses.numpy()).all()
    lerr = rel_err(losses.numpy(), want_l)
    print("saturated", dt.__name__, out_act, lerr)
    assert lerr < RTOL[dt]
    # gb of the last layer IS dz summed over the rows: numpy's is below 1e-80 in magnitude, the GPU's finite and as small
    assert np.abs(got[-1]).max() <= 1e-30 and np.abs(want_g[-1][1]).max() <= 1e-30
    _, recon, l2 = T.autoencoder_run(W, b, 1, x, out_act, "squaredError", "logistic", "tanh", want_code=False)
    assert loss_err(l2.numpy(), want_l) <= ATOL[dt]
    assert abs_err(recon.numpy(), AEN.run(ws, 1, X, "logistic", "tanh", out_act)[1]) <= ATOL[dt]
