"""Closed-loop generation in one call (to_rnn_stack_generate, csrc/rnn_generate.hip): prime a recurrent stack, then feed every
output back as the next input -- as stored, as its argMax one-hot, or as a symbol drawn by inverse CDF -- on both routes of
the generated steps (to_set_rnn_generate_persistent 0: per step, 2: the persistent kernel).

Correctness is checked by SELF-CONSISTENCY, not by comparing a closed loop with an independent closed loop (which amplifies
rounding, so no tolerance could be derived for it).  The decomposition is complete by induction:
  1. the feed rule, exactly: every symbol is the rule of tests/rnn_generate_numpy.py applied to the STORED row before it;
  2. open loop: with `fed` the inputs the call used (rebuilt from out / symbols), the call's outputs and final states are
     within the open-loop tolerance of tests/test_gpu_rnn_stack.py (1e-5 / 1e-11 relative per row) of the oracle's runNetwork
     stepped over concat(X, fed) -- identical inputs, nothing amplifies --, and on route 0 they are bit for bit chained
     to_rnn_stack_run calls at T = 1 that carry s_out into s.
The one-hot cases are "shift" stacks (GN.shift_stack) whose closed loop visits at least 3 symbols in every row; the seeds
are checked on the CPU by tests/test_rnn_generate_numpy_ref.py and the condition is asserted here on what the device fed.
Then: determinism, independence of a row from its batch, continuation, launches independent of G, routing, the contract and
non-finite inputs."""
import ctypes as C

import numpy as np
import pytest

import rnn_generate_numpy as GN
from test_rnn_generate_numpy_ref import CASES, oracle_open_loop, prime_data

pytestmark = pytest.mark.gpu
TOL = {np.float32: 1e-5, np.float64: 1e-11}   # tests/test_gpu_rnn_stack.py's
DTS = [np.float32, np.float64]
BY_NAME = {c[0]: c for c in CASES}


@pytest.fixture(scope="module")
def Ts():
    from tensor_ops_amd.hipt import HipT
    return {np.float32: HipT(0, np.float32), np.float64: HipT(0, np.float64)}


@pytest.fixture(autouse=True)
def auto_route():
    from tensor_ops_amd.hipt import HipT
    prev = HipT.rnn_generate_persistent(1)
    yield
    HipT.rnn_generate_persistent(prev)


def rel_err(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    den = np.linalg.norm(want.ravel())
    return np.linalg.norm((got - want).ravel()) / (den if den > 0 else 1.0)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def dev(T, layers):
    return [tuple(None if v is None else T.put(v) for v in lay[:4]) + (lay[4] if lay[4] else False,) for lay in layers]


def f64(layers):
    return [tuple(None if v is None else v.astype(np.float64) for v in lay[:4]) + (lay[4],) for lay in layers]


def put_seq(T, A, batched):
    return T.put(A, batched=True) if batched else T.put(A[0])


def generate(T, dl, X, G, feed, U, batched, out_act, hidden):
    """the call on X [B, Tp, i] (B = 1 and unbatched handles when not `batched`); every result as numpy with B in front"""
    nB, Tp = X.shape[:2]
    u = put_seq(T, U[:, :G], batched) if feed == "sample" else None
    out, sym, prime, fin = T.rnn_stack_generate(dl, put_seq(T, X, batched), G, feed, u, out_act, hidden,
                                                want_prime_out=True, want_states=True)
    assert (out.batch, prime.batch) == ((nB, nB) if batched else (0, 0))
    return {"out": out.numpy().reshape(nB, G, -1), "sym": sym, "prime": prime.numpy().reshape(nB, Tp, -1),
            "fin": [None if f is None else f.numpy().reshape(nB, -1) for f in fin], "fin_dev": fin}


def rebuild_fed(r, feed, U):
    """the inputs of the generated steps by the rule on the stored rows; asserts that the symbols are the rule's"""
    prev = np.concatenate([r["prime"][:, -1:], r["out"][:, :-1]], axis=1)
    fed = []
    for k in range(prev.shape[1]):
        x, c = GN.feed(prev[:, k], feed, U[:, k])
        fed.append(x)
        if c is None:
            assert r["sym"] is None
        else:
            assert np.array_equal(r["sym"][:, k], c), (k, r["sym"][:, k], c)
    return np.stack(fed, axis=1)


MODES = [(c, m) for c in CASES for m in (("output", "argmax", "sample") if c[3] == "softmax" else ("output",))]


@pytest.mark.parametrize("dt", DTS, ids=["f32", "f64"])
@pytest.mark.parametrize("route", [0, 2], ids=["per_step", "persistent"])
@pytest.mark.parametrize("case,feed", MODES, ids=lambda v: v[0] if isinstance(v, tuple) else v)
def test_feed_rule_and_open_loop(Ts, dt, route, case, feed):
    from tensor_ops_amd.hipt import HipT
    name, i, spec, out_act, hidden, seed = case
    T, tol = Ts[dt], TOL[dt]
    layers = GN.shift_stack(seed, i, spec, dt)
    dl, l64 = dev(T, layers), f64(layers)
    stateful = [l for l, lay in enumerate(layers) if lay[4]]
    HipT.rnn_generate_persistent(route)
    for B in (0, 7):
        for Tp in (1, 3):
            for G in (1, 12):
                nB = max(B, 1)
                X, U = prime_data(seed, nB, Tp, i, G, dt)
                p0 = HipT.rnn_generate_stats()
                r = generate(T, dl, X, G, feed, U, B > 0, out_act, hidden)
                p1 = HipT.rnn_generate_stats()
                assert (p1[0] - p0[0], p1[1] - p0[1]) == ((1, 0) if route == 2 else (0, 1))
                # 1. the feed rule, exactly
                fed = rebuild_fed(r, feed, U)
                if feed != "output" and G == 12:   # the closed loop walks: a constant sequence would test no wiring
                    assert min(len(set(row)) for row in r["sym"].tolist()) >= 3, r["sym"]
                # 2. open loop against the oracle, row by row and step by step
                allx = np.concatenate([X, fed], axis=1)
                errs = []
                for q in range(nB):
                    want, fin = oracle_open_loop(l64, hidden, out_act, allx[q])
                    got = np.concatenate([r["prime"][q], r["out"][q]])
                    errs += [rel_err(got[t], want[t]) for t in range(Tp + G)]
                    errs += [rel_err(r["fin"][l][q], st) for l, st in fin.items()]
                print(name, feed, B, Tp, G, "max open-loop error", max(errs))
                assert max(errs) < tol
                if route != 0:
                    continue
                # route 0: bit for bit chained to_rnn_stack_run calls at T = 1 that carry s_out into s
                cur = dl
                for t in range(Tp + G):
                    o, f = T.rnn_stack_run(cur, put_seq(T, allx[:, t:t + 1], B > 0), out_act, want_states=True, hidden_act=hidden)
                    got = r["prime"][:, t] if t < Tp else r["out"][:, t - Tp]
                    assert same_bits(o.numpy().reshape(nB, -1), got), (name, feed, B, Tp, G, t)
                    cur = [((f[l],) + lay[1:]) if lay[0] is not None else lay for l, lay in enumerate(cur)]
                for l in stateful:
                    assert same_bits(f[l].numpy().reshape(nB, -1), r["fin"][l])


@pytest.mark.parametrize("dt", DTS, ids=["f32", "f64"])
@pytest.mark.parametrize("route", [0, 2], ids=["per_step", "persistent"])
@pytest.mark.parametrize("feed", ["output", "argmax", "sample"])
def test_deterministic_and_independent_of_the_batch(Ts, dt, route, feed):
    from tensor_ops_amd.hipt import HipT
    name, i, spec, out_act, hidden, seed = BY_NAME["L2w"]   # 7 rows of 37 columns: two workgroups, the last one ragged
    T = Ts[dt]
    dl = dev(T, GN.shift_stack(seed, i, spec, dt))
    X, U = prime_data(seed, 7, 3, i, 12, dt)
    HipT.rnn_generate_persistent(route)
    a = generate(T, dl, X, 12, feed, U, True, out_act, hidden)
    b = generate(T, dl, X, 12, feed, U, True, out_act, hidden)
    for k in ("out", "prime"):
        assert same_bits(a[k], b[k])
    assert feed == "output" or np.array_equal(a["sym"], b["sym"])
    for l, f in enumerate(a["fin"]):
        assert f is None or same_bits(f, b["fin"][l])
    for q in (0, 4, 6):   # the same row alone
        one = generate(T, dl, X[q:q + 1], 12, feed, U[q:q + 1], False, out_act, hidden)
        assert same_bits(one["out"][0], a["out"][q]) and same_bits(one["prime"][0], a["prime"][q]), q
        assert feed == "output" or np.array_equal(one["sym"][0], a["sym"][q])
        for l, f in enumerate(a["fin"]):
            assert f is None or same_bits(one["fin"][l][0], f[q])


@pytest.mark.parametrize("dt", DTS, ids=["f32", "f64"])
@pytest.mark.parametrize("route", [0, 2], ids=["per_step", "persistent"])
@pytest.mark.parametrize("feed", ["output", "argmax", "sample"])
def test_continuation(Ts, dt, route, feed):
    """G = a + b in one call equals G = a, then a call primed with the ONE row feed(g_{a-1}) from the first call's s_out with
    G = b - 1 and the rest of U: its prime_out is g_a, its out g_{a+1} .., bit for bit"""
    from tensor_ops_amd.hipt import HipT
    name, i, spec, out_act, hidden, seed = BY_NAME["L3"]
    T = Ts[dt]
    dl = dev(T, GN.shift_stack(seed, i, spec, dt))
    a_, b_ = 5, 7
    X, U = prime_data(seed, 7, 3, i, a_ + b_, dt)
    HipT.rnn_generate_persistent(route)
    whole = generate(T, dl, X, a_ + b_, feed, U, True, out_act, hidden)
    first = generate(T, dl, X, a_, feed, U, True, out_act, hidden)
    assert same_bits(first["out"], whole["out"][:, :a_]) and same_bits(first["prime"], whole["prime"])
    x2, c2 = GN.feed(first["out"][:, -1], feed, U[:, a_])
    dl2 = [((first["fin_dev"][l],) + lay[1:]) if lay[0] is not None else lay for l, lay in enumerate(dl)]
    second = generate(T, dl2, x2[:, None, :], b_ - 1, feed, U[:, a_ + 1:], True, out_act, hidden)
    assert same_bits(second["prime"][:, 0], whole["out"][:, a_])
    assert same_bits(second["out"], whole["out"][:, a_ + 1:])
    if feed != "output":
        assert np.array_equal(c2, whole["sym"][:, a_]) and np.array_equal(second["sym"], whole["sym"][:, a_ + 1:])
    for l, f in enumerate(whole["fin"]):
        assert f is None or same_bits(second["fin"][l], f)


@pytest.mark.parametrize("dt", DTS, ids=["f32", "f64"])
def test_launches_do_not_depend_on_G(Ts, dt):
    from tensor_ops_amd.hipt import HipT
    name, i, spec, out_act, hidden, seed = BY_NAME["L3"]
    T = Ts[dt]
    dl = dev(T, GN.shift_stack(seed, i, spec, dt))

    def launches(G):
        X, U = prime_data(seed, 7, 3, i, G, dt)
        x = T.put(X, batched=True)
        T.rnn_stack_generate(dl, x, G, "argmax")
        l0 = T.stats()["launches"]
        T.rnn_stack_generate(dl, x, G, "argmax")
        return T.stats()["launches"] - l0
    HipT.rnn_generate_persistent(2)
    a, b = launches(4), launches(64)
    assert a == b, (a, b)
    HipT.rnn_generate_persistent(0)
    assert launches(4) < launches(8)   # the per-step route grows with G


def test_routing(Ts):
    """fp32 64 -> 128 (stateful) -> 64: 129 KiB of parameters, the persistent plan fits under 1 and 2; 64 -> 160 (stateful) ->
    64: 181 KiB of parameters alone, per step under every setting -- and still right"""
    from tensor_ops_amd.hipt import HipT
    T, dt = Ts[np.float32], np.float32
    B, Tp, G = 2, 1, 2
    for H, fits in ((128, True), (160, False)):
        layers = GN.shift_stack(21, 64, [(H, "logistic"), (64, None)], dt)
        dl, l64 = dev(T, layers), f64(layers)
        X, U = prime_data(21, B, Tp, 64, G, dt)
        for mode in (0, 1, 2):
            HipT.rnn_generate_persistent(mode)
            p0 = HipT.rnn_generate_stats()
            r = generate(T, dl, X, G, "argmax", U, True, "softmax", "logistic")
            p1 = HipT.rnn_generate_stats()
            assert (p1[0] - p0[0], p1[1] - p0[1]) == ((1, 0) if (fits and mode != 0) else (0, 1)), (H, mode)
            allx = np.concatenate([X, rebuild_fed(r, "argmax", U)], axis=1)
            for q in range(B):
                want, fin = oracle_open_loop(l64, "logistic", "softmax", allx[q])
                got = np.concatenate([r["prime"][q], r["out"][q]])
                assert max(rel_err(got[t], want[t]) for t in range(Tp + G)) < TOL[dt]
                assert rel_err(r["fin"][0][q], fin[0]) < TOL[dt]


def test_automatic_rule_is_bounded_in_B(Ts):
    """automatic = persistent while the batch fits 256 workgroups with at most four items of the widest layer a thread
    (include/tensorops_hip.h; measured in profiles/rnn_generate_scan.txt): fp32 64 -> 128 -> 64 up to B = 2048; forcing (2)
    ignores B"""
    from tensor_ops_amd.hipt import HipT
    T, dt = Ts[np.float32], np.float32
    dl = dev(T, GN.shift_stack(21, 64, [(128, "logistic"), (64, None)], dt))
    got = {}
    for B, mode, want in ((2048, 1, (1, 0)), (2049, 1, (0, 1)), (2049, 2, (1, 0))):
        X, U = prime_data(21, B, 1, 64, 2, dt)
        HipT.rnn_generate_persistent(mode)
        p0 = HipT.rnn_generate_stats()
        got[B, mode] = generate(T, dl, X, 2, "argmax", U, True, "softmax", "logistic")
        p1 = HipT.rnn_generate_stats()
        assert (p1[0] - p0[0], p1[1] - p0[1]) == want, (B, mode)
        rebuild_fed(got[B, mode], "argmax", U)   # (the feed rule on the stored rows, whichever route ran)


def test_contract(Ts):
    from tensor_ops_amd import capi
    from tensor_ops_amd.hipt import Graph, HipT
    L = capi.lib()
    T, dt = Ts[np.float32], np.float32
    name, i, spec, out_act, hidden, seed = BY_NAME["L2"]
    layers = GN.shift_stack(seed, i, spec, dt)
    dl = dev(T, layers)
    B, Tp, G = 3, 2, 2
    X, U = prime_data(seed, B, Tp, i, G, dt)
    x, u = T.put(X, batched=True), T.put(U, batched=True)
    pat = lambda *shape: T.put(np.full(shape, 7.5, dt), batched=True)  # noqa: E731
    out, prime, sfin = pat(B, G, i), pat(B, Tp, i), pat(B, 7)
    sym = np.full(B * G, -1, np.int64)

    def call(layers_=dl, xx=x, uu=None, g=G, feed=1, out_act_=2, oo=out, pp=prime, symbols=sym, sact=(0, -1)):
        n = len(layers_)
        arr = lambda k: (capi.c_tensor * n)(*[(lay[k].h if lay[k] is not None else None) for lay in layers_])  # noqa
        s_out = (capi.c_tensor * n)(sfin.h, None)
        return L.to_rnn_stack_generate(n, (C.c_int * n)(*sact), arr(0), arr(1), arr(2), arr(3), 0, out_act_, feed, xx.h,
                                       uu.h if uu is not None else None, g, pp.h if pp is not None else None, oo.h,
                                       symbols.ctypes.data_as(C.POINTER(C.c_int64)) if symbols is not None else None, s_out)
    narrow = GN.shift_stack(seed, i, [(7, "logistic"), (4, None)], dt)
    for route in (0, 2):
        HipT.rnn_generate_persistent(route)
        assert call(layers_=dev(T, narrow), oo=pat(B, G, 4), pp=pat(B, Tp, 4)) == 2   # n_L != i
        assert call(g=0) == 1                                                         # G = 0
        assert call(feed=2) == 1                                                      # SAMPLE without U
        assert call(feed=1, uu=u) == 1 and call(feed=0, uu=u, symbols=None) == 1      # U with another feed
        assert call(feed=0) == 1                                                      # symbols with OUTPUT
        assert call(out_act_=3) == 5                                                  # a tanh output activation
        assert call(oo=prime) == 1                                                    # out is prime_out (Tp == G)
        assert call(oo=x, pp=None) == 1                                               # out is X
        with Graph():
            st = call()
        assert st == 4                                                                # refused while a capture records
        for t in (out, prime, sfin):
            assert np.all(t.numpy() == dt(7.5))                                       # nothing was written
        assert np.all(sym == -1)
    assert call() == 0 and call(feed=2, uu=u) == 0 and call(feed=0, symbols=None) == 0
    assert np.all((sym >= 0) & (sym < i)) and not np.any(out.numpy() == dt(7.5))
    assert HipT.rnn_generate_persistent(1) in (0, 1, 2) and L.to_set_rnn_generate_persistent(3, None) == 1


@pytest.mark.parametrize("dt", DTS, ids=["f32", "f64"])
@pytest.mark.parametrize("route", [0, 2], ids=["per_step", "persistent"])
def test_non_finite(Ts, dt, route):
    """a NaN in one sequence's X: that row's outputs are NaN, its symbols stay in range, the other rows do not change"""
    from tensor_ops_amd.hipt import HipT
    name, i, spec, out_act, hidden, seed = BY_NAME["L2w"]
    T = Ts[dt]
    dl = dev(T, GN.shift_stack(seed, i, spec, dt))
    X, U = prime_data(seed, 7, 3, i, 12, dt)
    HipT.rnn_generate_persistent(route)
    clean = generate(T, dl, X, 12, "argmax", U, True, out_act, hidden)
    Xn = X.copy()
    Xn[3, 1, 2] = np.nan
    r = generate(T, dl, Xn, 12, "argmax", U, True, out_act, hidden)
    assert np.all(np.isnan(r["out"][3])) and np.all(np.isnan(r["prime"][3, 1:]))
    assert np.all((r["sym"] >= 0) & (r["sym"] < i))
    keep = [q for q in range(7) if q != 3]
    assert same_bits(r["out"][keep], clean["out"][keep]) and same_bits(r["prime"][keep], clean["prime"][keep])
    assert np.array_equal(r["sym"][keep], clean["sym"][keep])
