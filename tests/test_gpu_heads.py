"""Every softmax and loss row head of the library on one table of rows (tests/head_cases.py), against one float64 reference.

A row head is the per-row code behind a stack's last contraction.  It is written out in eight kernels: the fused head of the
16-wide tile (csrc/gemm_small.hip: the generic kernel and, behind a hidden layer of 256, the fp32 step kernel with its fused
tail), the joined forward + head launch (csrc/gemm_t32.hip: gemm_t32_head_kernel, from the planner under TOPS_STEP_SEAM=3 only),
loss_grad_rows_kernel (csrc/fused_fflayer.hip), the online recurrent head (csrc/rnn_online.hip), the induce head
(csrc/induce_seq.hip), the reconstruction head (csrc/recon_head.hip) and the two inference heads (csrc/infer_head.hip).

How a row reaches a head bit for bit.  One-layer stacks have K = n_L and W = 2 I, so z = 2 (x / 2) = the table's row (the
products with the zeros are exact); a non-finite logit comes from the bias and a non-finite target from y, never from x, where a
contraction would spread it over the row (0 * inf).  Stacks with a hidden layer have W_1 = 0 and b_1 = 0, so every hidden unit
is logistic(0) = 1/2 exactly, and rows of W_2 that sum to zero: z = 0 + b_2 is the table's row for every row of the batch and the
targets differ from row to row; the autoencoder, whose target is its input, gets its logits the same way.

What is held: p and dz to the absolute 1e-5 / 1e-12 of tests/test_gpu_infer.py, per-row losses as tests/test_gpu_autoencoder.py's
loss_err measures them to the same bounds, parameter gradients to the relative 1e-5 / 1e-11 of tests/test_gpu_stack_tanh.py;
where the reference is not finite, the same class (NaN, +inf, -inf) in the same places (nonfinite_ref.same_class_and_value on
the class of every element).  Every result lands in memory that held NaN (nan_pool), so an element no thread writes shows.  Each
test proves the head it means from the call's launch count, the routing query and the two-route entries' counters."""
import numpy as np
import pytest

import head_cases as HC
import nonfinite_ref as NR

pytestmark = pytest.mark.gpu
DTS = [np.float32, np.float64]
RTOL = {np.float32: 1e-5, np.float64: 1e-11}      # tests/test_gpu_stack_tanh.py: grad / sgd
ATOL = {np.float32: 1e-5, np.float64: 1e-12}      # tests/test_gpu_infer.py, tests/test_gpu_autoencoder.py: p, dz, losses


@pytest.fixture(scope="module")
def Ts():
    from tensor_ops_amd.hipt import HipT
    return {np.float32: HipT(0, np.float32), np.float64: HipT(0, np.float64)}


def ident(v):
    return getattr(v, "__name__", str(v))


def nan_pool(T, *counts):
    """upload and release NaN tensors of the sizes about to be asked for (tests/test_gpu_ewise_routes.py::nan_pool): the pool
    memory handed out next is NaN"""
    held = [T.put(np.full(int(n), np.nan, T.dtype.type)) for n in counts if n > 0]
    T.sync()
    del held


def counted(T, f):
    n0 = T.stats()["launches"]
    r = f()
    return r, T.stats()["launches"] - n0


class Report:
    """collects what differs, so that one run names every case a head misses"""

    def __init__(self, dt):
        self.dt, self.fails, self.worst = dt, [], {}

    def hold(self, ctx, what, got, want, how):
        """the class of every element (nonfinite_ref.same_class_and_value on the arrays with their finite elements zeroed), then
        the finite elements: how = "abs", "loss" (the difference over max(1, largest loss)) or "rel" (norms)"""
        g, w = np.asarray(got, np.float64), np.asarray(want, np.float64)
        assert g.shape == w.shape, (ctx, what, g.shape, w.shape)
        fin = np.isfinite(w)
        if not NR.same_class_and_value(np.where(np.isfinite(g), 0.0, g), np.where(fin, 0.0, w)):
            self.fails.append("%s %s: class %s" % (ctx, what, NR.describe(g, w, 3)))
            return
        if not fin.any():
            return
        wf = np.where(fin, w, 0.0)
        d = np.where(fin, g, 0.0) - wf
        if how == "abs":
            err, bound = np.abs(d).max(), ATOL[self.dt]
        elif how == "loss":
            err, bound = np.abs(d).max() / max(1.0, np.abs(wf).max()), ATOL[self.dt]
        else:
            err, bound = np.linalg.norm(d.ravel()) / max(np.linalg.norm(wf.ravel()), 1e-300), RTOL[self.dt]
        self.worst[what] = max(self.worst.get(what, 0.0), float(err))
        if not err <= bound:
            self.fails.append("%s %s: %s error %.3g > %g" % (ctx, what, how, err, bound))

    def done(self, name):
        print(name, np.dtype(self.dt).name, "worst", {k: "%.2g" % v for k, v in self.worst.items()}, "failures", len(self.fails))
        for f in self.fails:
            print("  MISS", f)
        assert not self.fails, "%d misses, the first: %s" % (len(self.fails), self.fails[:4])


def grads_ref(dz, X):
    """(gW, gb) = (dz^T X, the row sums of dz) in IEEE arithmetic"""
    return NR.contract(dz.T, X), NR.sum_rows(dz)


def row_batches(n, dt, sizes=HC.BATCHES):
    """(id, X rows with z = 2 x, bias, Y) of every batch: the table's, then the special ones"""
    out = []
    for b in HC.batches(HC.finite_cases(n, dt), sizes):
        out.append((b[0]["id"] + "+%d" % (len(b) - 1), np.stack([c["z"] for c in b]) / 2.0, np.zeros(n), np.stack([c["y"] for c in b])))
    for c in HC.special_batches(n, dt):
        out.append((c["id"], c["x"] / 2.0, c["bias"], c["y"]))
    return out


def shared_batches(n, dt, head="softmax"):
    """(id, the logit row every row of the batch gets, Y): each pattern x spread with 5, 7, 1 target rows in turn, then the
    special ones"""
    spreads = HC.SPREADS if head == "softmax" else HC.SE_SPREADS
    ys = [HC.target(k, n, i) for i, k in enumerate(HC.TARGETS)] + [HC.target("onehot", n, 5), HC.target("onehot", n, 6)]
    out, i = [], 0
    for s in spreads:
        for pat in HC.PATTERNS:
            B = (5, 7, 1)[i % 3]
            Y = np.stack(ys[:B]) if B > 1 else np.stack([ys[4]])
            out.append(("%s-%g-n%d-B%d" % (pat, s, n, B), HC.logits(pat, s, n, dt), HC.stored(Y, dt)))
            i += 1
    if head == "softmax":
        for c in HC.special_batches(n, dt):
            out.append((c["id"], c["x"][0] + c["bias"], c["y"]))
    return out


# ---- 1. to_fflayer_stack_grad, one layer: the fused head up to 16 logits, loss_grad_rows_kernel beyond -------------------------
@pytest.mark.parametrize("dt", DTS, ids=ident)
@pytest.mark.parametrize("n", HC.WIDTHS["fused"] + HC.WIDTHS["rows"])
def test_stack_grad_one_layer(Ts, n, dt):
    T, rep = Ts[dt], Report(dt)
    fused = n <= 16
    W = 2.0 * np.eye(n)
    for cid, X, bias, Y in row_batches(n, dt):
        B = len(X)
        if fused:   # the head is fused on the small-GEMM route alone
            q = T.gemm_route(B, n, n, dtype="f64" if dt == np.float64 else "f32", b_transposed=True, epilogue=("bias",))
            assert q["small_route"], (cid, q)
        w, b, x, y = T.put(W), T.put(bias), T.put(X, batched=True), T.put(Y, batched=True)
        nan_pool(T, n * n, n, B, B * n)
        (gW, gb, losses), k = counted(T, lambda: T.stack_grad([w], [b], x, y, want_losses=True))
        # the forward (with the fused head, or followed by the head's own launch) and one weight-gradient launch
        assert k == (2 if fused else 3), (cid, k)
        _, dz, loss = HC.softmax_ce(2.0 * X + bias, Y)
        want_gW, want_gb = grads_ref(dz, X)
        rep.hold(cid, "loss", losses.numpy(), loss, "loss")
        rep.hold(cid, "gW", gW[0].numpy(), want_gW, "rel")
        rep.hold(cid, "gb", gb[0].numpy(), want_gb, "rel")
        if B == 1:
            rep.hold(cid, "dz", gb[0].numpy(), dz[0], "abs")     # one row: gb IS dz
    rep.done("stack_grad one layer n=%d (%s)" % (n, "fused head" if fused else "loss_grad_rows"))


# ---- 2. behind a hidden layer: the fused tail's cotangent as well ---------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS, ids=ident)
@pytest.mark.parametrize("n,hidden", [(10, 8), (16, 8), (16, 256), (10, 256), (17, 8)])
def test_stack_grad_behind_a_hidden_layer(Ts, n, hidden, dt):
    """hidden = 256 in fp32 is the benchmarked step's shape class: the lean step kernel with the tail fused behind the head"""
    T, rep = Ts[dt], Report(dt)
    i0 = 12
    rng = np.random.default_rng(n * 1000 + hidden)
    W2 = rng.integers(-3, 4, (n, hidden)).astype(np.float64)
    W2[:, -1] -= W2.sum(axis=1)                       # rows that sum to zero: W_2 (1/2, ..., 1/2) = 0 exactly
    assert (W2.sum(axis=1) == 0).all() and np.abs(W2).max() <= 3 * hidden
    H = np.full((7, hidden), 0.5)
    counts = set()
    for cid, zrow, Y in shared_batches(n, dt):
        B = len(Y)
        X = rng.integers(-4, 5, (B, i0)).astype(np.float64)
        if n <= 16:   # the head is fused on the small-GEMM route alone
            q = T.gemm_route(B, hidden, n, dtype="f64" if dt == np.float64 else "f32", b_transposed=True, epilogue=("bias",))
            assert q["small_route"], (cid, q)
        ws = [T.put(np.zeros((hidden, i0))), T.put(W2)]
        bs = [T.put(np.zeros(hidden)), T.put(zrow)]
        x, y = T.put(X, batched=True), T.put(Y, batched=True)
        nan_pool(T, hidden * i0, n * hidden, hidden, n, B, B * n, B * hidden)
        (gW, gb, losses), k = counted(T, lambda: T.stack_grad(ws, bs, x, y, want_losses=True))
        counts.add((B == 1, k))
        _, dz, loss = HC.softmax_ce(np.broadcast_to(zrow, Y.shape), Y)
        want_gW2, want_gb2 = grads_ref(dz, H[:B])
        dz1 = 0.25 * NR.contract(dz, W2)                 # the reference's dz pushed back: (dz W_2) h (1 - h), h = 1/2
        want_gW1, want_gb1 = grads_ref(dz1, X)
        rep.hold(cid, "loss", losses.numpy(), loss, "loss")
        for name, g, want in (("gW2", gW[1], want_gW2), ("gb2", gb[1], want_gb2), ("gW1", gW[0], want_gW1), ("gb1", gb[0], want_gb1)):
            rep.hold(cid, name, g.numpy(), want, "rel")
    # The launches of a step do not depend on the values.  Two forwards; the head's own launch unless it is fused (n <= 16); the
    # backward contraction unless the tail is fused behind the head (a hidden layer of eight 16-column chunks or more); the weight
    # gradients: one rank-1 launch for a single row, else the fp32 pair's one launch or fp64's two.
    print("launches", n, hidden, np.dtype(dt).name, sorted(counts))
    fused, tail = n <= 16, n <= 16 and hidden >= 128
    base = 2 + (0 if fused else 1) + (0 if tail else 1)
    assert counts == {(True, base + 1), (False, base + (1 if dt == np.float32 else 2))}, counts
    rep.done("stack_grad %d-%d behind a hidden layer" % (hidden, n))


# ---- 3. the inference heads ------------------------------------------------------------------------------------------------------
def check_infer(T, rep, cid, out, cls, conf, Z, Y, tie_free):
    p, _, _ = HC.softmax_ce(Z, Y)
    rep.hold(cid, "p", out, p, "abs")
    stored_cls = T.arg_max(T.put(out, batched=True))
    if not np.array_equal(cls, stored_cls):
        rep.fails.append("%s classes %s, to_arg_max of the stored rows %s" % (cid, cls, stored_cls))
    want_cls = np.argmax(Z, axis=1)
    if not np.array_equal(cls[tie_free], want_cls[tie_free]):
        rep.fails.append("%s classes %s, the reference's %s on the tie-free rows" % (cid, cls[tie_free], want_cls[tie_free]))
    actual = T.arg_max(T.put(Y, batched=True))
    n = Z.shape[1]
    want = np.zeros((n, n), np.int64)
    np.add.at(want, (cls, actual), 1)
    if not np.array_equal(conf, want):
        rep.fails.append("%s confusion matrix" % cid)


def infer_batches(n, dt):
    out = []
    for b in HC.batches(HC.finite_cases(n, dt)):
        Z = np.stack([c["z"] for c in b])
        out.append((b[0]["id"] + "+%d" % (len(b) - 1), Z / 2.0, np.zeros(n), np.stack([c["y"] for c in b]),
                    np.array([c["tie_free"] for c in b])))
    for c in HC.special_batches(n, dt):
        out.append((c["id"], c["x"] / 2.0, c["bias"], c["y"], np.zeros(len(c["x"]), bool)))
    return out


@pytest.mark.parametrize("dt", DTS, ids=ident)
@pytest.mark.parametrize("n", sorted(set(HC.WIDTHS["narrow"] + HC.WIDTHS["rows"])))
def test_infer_heads(Ts, n, dt):
    """infer_narrow_kernel up to 32 logits (a one-layer net is the whole call in one launch), infer_rows_kernel beyond (the
    contraction, then the head)"""
    T, rep = Ts[dt], Report(dt)
    W = 2.0 * np.eye(n)
    for cid, X, bias, Y, tie_free in infer_batches(n, dt):
        w, b, x, y = T.put(W), T.put(bias), T.put(X, batched=True), T.put(Y, batched=True)
        nan_pool(T, len(X) * n, len(X), n * n)
        (out, cls, conf), k = counted(T, lambda: T.infer_stack([w], [b], x, y=y, want_out=True))
        assert k == (1 if n <= 32 else 2), (cid, k)
        check_infer(T, rep, cid, out.numpy(), cls, conf, 2.0 * X + bias, Y, tie_free)
    rep.done("infer n=%d (%s)" % (n, "narrow" if n <= 32 else "rows"))


@pytest.mark.parametrize("dt", DTS, ids=ident)
@pytest.mark.parametrize("n", [17, 65])
def test_rnn_run_head(Ts, n, dt):
    """to_rnn_stack_run's head is infer_rows_kernel at every width (a stateless layer: the bias is added by the head)"""
    T, rep = Ts[dt], Report(dt)
    W = 2.0 * np.eye(n)
    for cid, X, bias, Y, tie_free in infer_batches(n, dt):
        lay = [(None, None, T.put(W), T.put(bias))]
        x = T.put(X[:, None, :], batched=True)
        nan_pool(T, len(X) * n, len(X) * n)
        (out, _), k = counted(T, lambda: T.rnn_stack_run(lay, x))
        # the contraction (without its bias) and infer_rows_kernel; with several sequences the rows go into time-major order
        # first and back afterwards, one launch each
        assert k == (2 if len(X) == 1 else 4), (cid, k)
        Z = 2.0 * X + bias
        p, _, _ = HC.softmax_ce(Z, Y)
        got = out.numpy()[:, 0, :]
        rep.hold(cid, "p", got, p, "abs")
        # (the entry hands out no classes: those of the stored rows, on the rows where the largest logit comes once)
        cls = T.arg_max(T.put(got, batched=True))
        if not np.array_equal(cls[tie_free], np.argmax(Z, axis=1)[tie_free]):
            rep.fails.append("%s classes of the stored rows %s" % (cid, cls))
    rep.done("rnn_stack_run n=%d" % n)


# ---- 4. the reconstruction head -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS, ids=ident)
@pytest.mark.parametrize("out_act", ["softmax", "logistic", "tanh", "identity"])
@pytest.mark.parametrize("n", HC.WIDTHS["recon"])
def test_reconstruction_head(Ts, n, out_act, dt):
    """to_autoencoder_stack_run: the target of a row is the row itself, the logits come from the decoder's bias behind a code of
    zeros (W_1 = 0, no code activation).  A row with a NaN in it has NaN logits too: 0 * NaN in the encoder."""
    T, rep = Ts[dt], Report(dt)
    c = 5
    loss = "crossEntropy" if out_act == "softmax" else "squaredError"
    W2 = np.arange(n * c).reshape(n, c) % 7 - 3.0
    for cid, zrow, Y in shared_batches(n, dt, out_act):
        B = len(Y)
        ws, bs = [T.put(np.zeros((c, n))), T.put(W2)], [T.put(np.zeros(c)), T.put(zrow)]
        x = T.put(Y, batched=True)
        _, k_code = counted(T, lambda: T.autoencoder_run(ws, bs, 1, x, out_act, loss, "logistic", "identity", want_recon=False,
                                                         want_losses=False))
        nan_pool(T, B * c, B * n, B)
        (code, recon, losses), k = counted(T, lambda: T.autoencoder_run(ws, bs, 1, x, out_act, loss, "logistic", "identity"))
        assert k == k_code + 2, (cid, k, k_code)             # the decoder's contraction and the head
        Z = np.where(np.isfinite(Y).all(axis=1)[:, None], zrow[None, :], np.nan)
        a, _, want_loss = HC.HEADS[out_act](Z, Y)
        rep.hold(cid, "p", recon.numpy(), a, "abs")
        rep.hold(cid, "loss", losses.numpy(), want_loss, "loss")
    rep.done("recon head %s n=%d" % (out_act, n))


@pytest.mark.parametrize("dt", DTS, ids=ident)
@pytest.mark.parametrize("n", HC.WIDTHS["recon"])
def test_autoencoder_grad_heads(Ts, n, dt):
    """to_autoencoder_stack_grad on the same rows: the cotangent each head stores, seen through the gradients.  The code is
    b_1 = (1, ..., 1) behind W_1 = 0 with no code activation, the rows of W_2 sum to zero, b_2 is the table's row: gb_2 is the row
    sum of dz (dz itself for a single row), gW_2 = dz^T code, and gW_1, gb_1 carry dz W_2.  The step routes by pair
    (StackStep::launch): tanh and identity go through the reconstruction head with dz written over z, one launch behind the
    contraction; softmax and logistic take the heads of to_fflayer_stack_grad -- fused up to 16 logits, loss_grad_rows_kernel
    beyond -- so the reconstruction head's dz store of those two pairs is reached by no entry.  Sums of at most seven rows are
    measured as the losses are, the difference over max(1, largest element): a saturated tanh's cotangent is 1e-13 in float64
    and exactly 0 in fp32, and a norm-relative bound on a gradient that small would measure nothing."""
    T, rep = Ts[dt], Report(dt)
    c = 5
    W2 = np.arange(n * c).reshape(n, c) % 7 - 3.0
    W2[:, -1] -= W2.sum(axis=1)
    counts = {}
    for out_act in ("softmax", "logistic", "tanh", "identity"):
        loss = "crossEntropy" if out_act == "softmax" else "squaredError"
        for cid, zrow, Y in shared_batches(n, dt, out_act):
            B = len(Y)
            ws, bs = [T.put(np.zeros((c, n))), T.put(W2)], [T.put(np.ones(c)), T.put(zrow)]
            x = T.put(Y, batched=True)
            nan_pool(T, c * n, n * c, c, n, B, B * n, B * c)
            (gW, gb, losses), k = counted(T, lambda: T.autoencoder_grad(ws, bs, 1, x, out_act, loss, "logistic", "identity",
                                                                        want_losses=True))
            counts.setdefault((out_act, B == 1), set()).add(k)
            clean = np.isfinite(Y).all(axis=1)[:, None]
            Z = np.where(clean, zrow[None, :], np.nan)                 # (0 * NaN in the encoder: the row's code is NaN)
            code = np.where(clean, np.ones((B, c)), np.nan)
            _, dz, want_loss = HC.HEADS[out_act](Z, Y)
            dcode = NR.contract(dz, W2)
            ctx = "%s %s" % (out_act, cid)
            rep.hold(ctx, "loss", losses.numpy(), want_loss, "loss")
            for name, g, want in (("gW2", gW[1], NR.contract(dz.T, code)), ("gb2", gb[1], NR.sum_rows(dz)),
                                  ("gW1", gW[0], NR.contract(dcode.T, Y)), ("gb1", gb[0], NR.sum_rows(dcode))):
                rep.hold(ctx, name, g.numpy(), want, "loss")
            if B == 1:
                rep.hold(ctx, "dz", gb[1].numpy(), dz[0], "loss")
    print("launches", n, np.dtype(dt).name, {k: sorted(v) for k, v in counts.items()})
    for one in (False, True):
        ks = {a: counts[(a, one)] for a in ("softmax", "logistic", "tanh", "identity")}
        assert all(len(v) == 1 for v in ks.values()), counts
        k = {a: min(v) for a, v in ks.items()}
        # the reconstruction head and loss_grad_rows_kernel are one launch behind the contraction, the fused head is none
        assert k["tanh"] == k["identity"] and k["softmax"] == k["logistic"] == k["tanh"] - (1 if n <= 16 else 0), counts
    rep.done("autoencoder_grad n=%d" % n)


# ---- 5. the entries with two routes: both on the same rows, each against the reference, their NaN masks against each other --------
def two_routes(T, rep, cid, switch, stats, run):
    """run() under the switch at 0 and at 2; the counters say which route ran; returns {mode: result}"""
    got = {}
    for mode, slot in ((0, 1), (2, 0)):
        prev = switch(mode)
        try:
            s0 = stats()
            got[mode] = run(mode)
            s1 = stats()
        finally:
            switch(prev)
        delta = [b - a for a, b in zip(s0, s1)]
        assert delta[slot] == 1 and delta[1 - slot] == 0, (cid, mode, s0, s1)
    for k in got[0]:
        if not np.array_equal(np.isnan(got[0][k]), np.isnan(got[2][k])):
            rep.fails.append("%s %s: the two routes' NaN masks differ: %s" % (cid, k, NR.describe(got[2][k], got[0][k], 3)))
    return got


@pytest.mark.parametrize("dt", DTS, ids=ident)
@pytest.mark.parametrize("n", HC.WIDTHS["wave"])
def test_induce_both_routes(Ts, n, dt):
    """to_fflayer_stack_induce, one iteration: loss_grad_rows_kernel per iteration, the wave head of induce_seq.hip persistently"""
    T, rep = Ts[dt], Report(dt)
    W, rate = 2.0 * np.eye(n), 0.125
    for cid, X, bias, Y in row_batches(n, dt):
        B = len(X)
        _, dz, loss = HC.softmax_ce(2.0 * X + bias, Y)

        def run(mode):
            w, b, x, y = T.put(W), T.put(bias), T.put(X, batched=True), T.put(Y, batched=True)
            nan_pool(T, B * n, B * n, B)
            out, gx, ls = T.induce_stack([w], [b], x, y, rate, 1, want_gx=True, want_losses=True)
            return {"out": out.numpy(), "gx": gx.numpy(), "loss": ls.numpy()[:, 0]}

        got = two_routes(T, rep, cid, T.induce_persistent, T.induce_stats, run)
        for mode, r in got.items():
            ctx = "%s route %s" % (cid, "A" if mode == 0 else "B")
            rep.hold(ctx, "loss", r["loss"], loss, "loss")
            rep.hold(ctx, "dz", r["gx"] / 2.0, dz, "abs")       # gx = dz W = 2 dz
            rep.hold(ctx, "out", r["out"], X - rate * 2.0 * dz, "rel")
    rep.done("induce n=%d" % n)


def rnn_layer(T, n, bias):
    """one stateful layer with W' = 0 and the initial state 0: z_t = 2 x_t + 0 s_t + b"""
    return [(T.put(np.zeros(n)), T.put(np.zeros((n, n))), T.put(2.0 * np.eye(n)), T.put(bias))]


@pytest.mark.parametrize("dt", DTS, ids=ident)
@pytest.mark.parametrize("n", [17, 65])
def test_rnn_grad_both_routes(Ts, n, dt):
    """to_rnn_stack_grad: the head is loss_grad_rows_kernel over all B * T rows on both routes of the recurrence.  Two steps a
    sequence on the table's rows; one step on the special ones (a NaN cotangent would travel through 0 * NaN to the step before)"""
    T, rep = Ts[dt], Report(dt)
    for cid, X, bias, Y in row_batches(n, dt, sizes=(14, 10, 2)):
        steps = 2 if np.isfinite(bias).all() and np.isfinite(Y).all() else 1
        B = len(X) // steps
        X3, Y3 = X.reshape(B, steps, n), Y.reshape(B, steps, n)
        _, dz, loss = HC.softmax_ce(2.0 * X + bias, Y)
        want_gW, want_gb = grads_ref(dz, X)

        def run(mode):
            lay = rnn_layer(T, n, bias)
            x, y = T.put(X3, batched=True), T.put(Y3, batched=True)
            nan_pool(T, B * steps * n, B * steps * n, B * steps, n * n, n)
            _, _, gw, gb, gx, ls = T.rnn_stack_grad(lay, x, y, want_gx=True, want_losses=True)
            return {"gx": gx.numpy().reshape(-1, n), "loss": ls.numpy().reshape(-1), "gW": gw[0].numpy(), "gb": gb[0].numpy()}

        got = two_routes(T, rep, cid, T.rnn_persistent, T.rnn_stats, run)
        for mode, r in got.items():
            ctx = "%s mode %d" % (cid, mode)
            rep.hold(ctx, "loss", r["loss"], loss, "loss")
            rep.hold(ctx, "dz", r["gx"] / 2.0, dz, "abs")
            rep.hold(ctx, "gW", r["gW"], want_gW, "rel")
            rep.hold(ctx, "gb", r["gb"], want_gb, "rel")
    rep.done("rnn_stack_grad n=%d" % n)


@pytest.mark.parametrize("dt", DTS, ids=ident)
@pytest.mark.parametrize("n", [17, 65])
def test_rnn_online_both_routes(Ts, n, dt):
    """to_rnn_stack_online_sgd on one sequence whose steps are the rows, both rates 1: the parameters move by the gradients (b
    from 0 to -gb, W from 2 I to 2 I - gW).  loss_grad_rows_kernel per sequence, the head of rnn_online.hip persistently.  The
    row with a NaN target is a sequence of its own (see test_rnn_grad_both_routes)."""
    T, rep = Ts[dt], Report(dt)
    calls = []
    for cid, X, bias, Y in row_batches(n, dt):
        if np.isfinite(Y).all():
            calls.append((cid, X, bias, Y))
        else:
            calls += [("%s row %d" % (cid, r), X[r:r + 1], bias, Y[r:r + 1]) for r in range(len(X))]
    for cid, X, bias, Y in calls:
        steps = len(X)
        _, dz, loss = HC.softmax_ce(2.0 * X + bias, Y)
        want_gW, want_gb = grads_ref(dz, X)

        def run(mode):
            lay = rnn_layer(T, n, bias)
            x, y = T.put(X[None], batched=True), T.put(Y[None], batched=True)
            nan_pool(T, steps, steps * n)
            ls = T.rnn_stack_online_sgd(lay, x, y, 1.0, 1.0, want_losses=True)
            return {"loss": ls.numpy().reshape(-1), "W": lay[0][2].numpy(), "b": lay[0][3].numpy()}

        got = two_routes(T, rep, cid, T.rnn_online_persistent, T.rnn_online_stats, run)
        for mode, r in got.items():
            ctx = "%s mode %d" % (cid, mode)
            rep.hold(ctx, "loss", r["loss"], loss, "loss")
            rep.hold(ctx, "W", r["W"], 2.0 * np.eye(n) - want_gW, "rel")
            rep.hold(ctx, "b", r["b"], bias - want_gb, "rel")
            if steps == 1 and np.isfinite(bias).all():
                rep.hold(ctx, "dz", -r["b"], dz[0], "abs")       # one step from b = 0: -b IS dz
    rep.done("rnn_stack_online_sgd n=%d" % n)


# ---- 6. the planner's heads, with a loss node: the fused head by default, the joined forward + head launch under its switch -----
def test_planner_heads_with_a_loss_node(repo_root):
    """tests/head_plan_child.py in two fresh processes (the library reads TOPS_STEP_SEAM once, at start): a recorded training
    step of config 3's shape class with the loss asked for beside the gradients, on the table's rows.  By default the head is
    gemm_small.hip's, fused behind the second layer; under TOPS_STEP_SEAM=3 the first layer and the head are ONE launch,
    gemm_t32_head_kernel -- one launch fewer a step.  Both are held to the reference, losses and gradients."""
    import json
    import os
    import subprocess
    import sys
    got = {}
    for seam in ("0", "3"):
        env = dict(os.environ, TOPS_STEP_SEAM=seam, PYTHONPATH=repo_root)
        r = subprocess.run([sys.executable, os.path.join(repo_root, "tests", "head_plan_child.py")], env=env, capture_output=True,
                           text=True, timeout=300, cwd=repo_root)
        assert r.returncode == 0, r.stderr[-3000:]
        got[seam] = json.loads(r.stdout.strip().splitlines()[-1])
        print("planner heads, TOPS_STEP_SEAM=" + seam, got[seam]["launches"], got[seam]["worst"], len(got[seam]["fails"]))
        for f in got[seam]["fails"]:
            print("  MISS", f)
    for n in ("10", "16"):
        a, b = got["0"]["launches"][n], got["3"]["launches"][n]
        assert len(a) == 1 and len(b) == 1 and b[0] == a[0] - 1, (n, a, b)
    assert not got["0"]["fails"] and not got["3"]["fails"], (got["0"]["fails"][:4], got["3"]["fails"][:4])
