"""The reduction, layout and argMax kernels of csrc/reduce_layout.hip, route by route (tables, restated routing and
references: tests/reduce_layout_cases.py).

Sums run on integers in -5 .. 5 and layout on `arange`, so every comparison is bit-exact and a dropped, doubled or misplaced
element shows; each sum route also gets one pass on random data under the project's bound (1e-5 / 1e-12 of the sum of
magnitudes).  The launch counter checks that a case took the route the restatement says.  One case per sum route and every
gather run on a view of the interior of a NaN-filled tensor that starts at an element offset which is no multiple of 4
wherever the row size allows one: a NaN in the result is a read outside the view.  argMax / argMin are held to
`oracle.tensor`'s left fold row by row, NaN included, and so are the two stack kernels that restate them.  Everything is an
eager call outside any memo scope."""
import ctypes as C
import json
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

import reduce_layout_cases as RC

pytestmark = pytest.mark.gpu
DTS = [np.float32, np.float64]
IDS = ["f32", "f64"]
BOUND = {np.float32: 1e-5, np.float64: 1e-12}   # README / test_big_reductions: |error| <= BOUND * sum |x|
NAN_COLUMNS = lambda n: [[0], [n // 2], [n - 1], [3, 67] if n > 67 else [1, n - 2], [1, n // 3, n - 3]]   # noqa: E731


@pytest.fixture(scope="module")
def backends():
    from tensor_ops_amd.hipb import HipB
    return {dt: HipB(0, dtype=dt) for dt in DTS}


def seed_of(name):
    return zlib.crc32(name.encode())


def nan_surround(T, x, B):
    """a handle on x (B > 0: batched, x [B, ...]) that is a view of the interior of a NaN-filled tensor; starts numel in"""
    big = np.full(((B if B else 1) + 2,) + x.shape[(1 if B else 0):], np.nan, dtype=x.dtype)
    big[1:-1] = x if B else x[None]
    d = T.put(big, batched=True)
    return T.batch_slice(d, 1, B) if B else T.batch_select(d, 1)


# ---- (a) sums ------------------------------------------------------------------------------------------------------------
def check_sum(Bl, dt, case, gemv_on=True, integers=True):
    T = Bl.T
    route = case["route"] if gemv_on else case["off_route"]
    x = RC.sum_data(case, dt, np.random.default_rng(seed_of(case["id"])), integers)
    got, launches = RC.run_sum_case(T, Bl, case, x)
    want, mag = RC.sum_reference(case, x)
    got = np.asarray(got, np.float64)
    assert got.shape == np.shape(want), (case["id"], got.shape, np.shape(want))
    err = float(np.max(np.abs(got - want) / np.maximum(mag, 1e-300))) if got.size else 0.0
    print(case["id"], np.dtype(dt).name, route, "launches", launches, "max error / sum|x|", err)
    if integers:
        assert np.array_equal(got, want), case["id"]
    else:
        assert np.all(np.abs(got - want) <= BOUND[dt] * mag), (case["id"], err)
    assert launches in RC.SUM_LAUNCHES[route], (case["id"], route, launches)
    return route


@pytest.mark.parametrize("dt", DTS, ids=IDS)
@pytest.mark.parametrize("case", RC.SUM_CASES, ids=[c["id"] for c in RC.SUM_CASES])
def test_sum_route_exact(backends, dt, case):
    check_sum(backends[dt], dt, case)


@pytest.mark.parametrize("dt", DTS, ids=IDS)
def test_sum_over_a_batch_past_grid_y(backends, dt):
    """sumRows of [B = 65537; R, 64]: the batch is the column kernel's grid.y"""
    check_sum(backends[dt], dt, RC.grid_y_case(dt))


@pytest.mark.parametrize("dt", DTS, ids=IDS)
def test_sum_routes_random_data(backends, dt):
    """one case a route (the view where there is one) on uniform(-1, 1) data, under the README's bound"""
    seen = set()
    for case in sorted(RC.SUM_CASES, key=lambda c: not c["view"]):
        if case["route"] not in seen and case["route"] != "fill":
            seen.add(check_sum(backends[dt], dt, case, integers=False))
    assert seen == set(RC.SUM_ROUTES) - {"none", "fill"}


@pytest.mark.parametrize("dt", DTS, ids=IDS)
@pytest.mark.parametrize("n", [65536, 70001])
def test_dot_of_long_vectors_exact(backends, dt, n):
    """to_blas_dot is a contraction (gemv.hip or the small-GEMM kernel), not launch_sum_axis: held to the same data and
    exactness at the sizes where a single reduction changes kernels"""
    Bl = backends[dt]
    rng = np.random.default_rng(n)
    x, y = rng.integers(-5, 6, n).astype(dt), rng.integers(-5, 6, n).astype(dt)
    assert Bl.dot(Bl.T.put(x), Bl.T.put(y)) == float(x.astype(np.float64) @ y.astype(np.float64))
    assert Bl.dot(nan_surround(Bl.T, x, 0), nan_surround(Bl.T, y, 0)) == float(x.astype(np.float64) @ y.astype(np.float64))


def _child_sums():
    """the body of the TOPS_GEMV=0 child: the whole sum table and the shapes gemv.hip takes otherwise; one JSON line"""
    from tensor_ops_amd.hipb import HipB
    out = []
    for dt in DTS:
        Bl = HipB(0, dtype=dt)
        for case in RC.sum_cases(dt) + RC.sum_extra_off_cases(dt):
            rec = {"id": case["id"], "dt": np.dtype(dt).name, "route": case["off_route"], "ok": False, "why": ""}
            try:
                check_sum(Bl, dt, case, gemv_on=False)
                rec["ok"] = True
            except AssertionError as e:
                rec["why"] = str(e)[-400:]
            out.append(rec)
    print(json.dumps(out))


def test_sum_routes_with_the_column_kernel_off(repo_root):
    """TOPS_GEMV=0 is read once a process: a fresh one runs the table; the two-pass, plain column, rows and partial routes
    take what launch_column_sum takes otherwise"""
    here = os.path.dirname(os.path.abspath(__file__))
    code = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_reduce_layout as t; t._child_sums()" % (repo_root, here)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, TOPS_GEMV="0"), capture_output=True, text=True,
                       timeout=600, cwd=repo_root)
    assert r.returncode == 0, r.stderr[-3000:]
    recs = json.loads(r.stdout.strip().splitlines()[-1])
    bad = [x for x in recs if not x["ok"]]
    assert not bad, bad
    assert len(recs) == sum(len(RC.sum_cases(dt)) + 4 for dt in DTS)
    for dt in IDS:
        assert {x["route"] for x in recs if x["dt"] == {"f32": "float32", "f64": "float64"}[dt]} == \
            set(RC.SUM_ROUTES) - {"none", "column_sum"}


# ---- (b) packing a strided view ----------------------------------------------------------------------------------------
def copy_operand(T, dt, case):
    """(handle of the transp view, host array it is the transpose of)"""
    B, shape = case["B"], case["shape"]
    x = np.arange(max(B, 1) * int(np.prod(shape)), dtype=dt).reshape(((B,) if B else ()) + shape)
    d = nan_surround(T, x, B) if case["view"] else T.put(x, batched=bool(B))
    return T.transp(d), x


@pytest.mark.parametrize("dt", DTS, ids=IDS)
@pytest.mark.parametrize("case", RC.COPY_CASES, ids=[c["id"] for c in RC.COPY_CASES])
def test_pack_of_a_transposed_view(backends, dt, case):
    T = backends[dt].T
    v, x = copy_operand(T, dt, case)
    want = RC.copy_reference(case, x)
    got = v.numpy()                                   # to_download packs the view
    assert got.shape == want.shape and np.array_equal(got, want), case["id"]
    # ... and so does an op that needs a packed operand: sumRows (transp x); its launches are the pack's one and the sum's
    dims, st = RC.copy_case_view(case)
    packed = RC.copy_route(dims, st) == "memcpy"      # (a view that is one run is packed already: contiguous() copies nothing)
    T.sync()
    before = T.stats()["launches"]
    s = T.sumRows(v)
    launches = T.stats()["launches"] - before
    ax = 1 if case["B"] else 0
    assert np.array_equal(s.numpy().astype(np.float64), want.astype(np.float64).sum(axis=ax)), case["id"]
    O, R, J = max(case["B"], 1), want.shape[ax], int(np.prod(want.shape[ax + 1:]))
    sums = RC.SUM_LAUNCHES[RC.sum_axis_route(O, R, J, 1)]
    print(case["id"], case["route"], "launches", launches)
    assert launches - (0 if packed else 1) in sums, (case["id"], launches)


@pytest.mark.parametrize("dt", DTS, ids=IDS)
def test_copy_of_one_packed_run(backends, dt):
    """the copy's memcpy route: `contiguous()` never asks for it (a view that is one run is packed), the stack entries do --
    to_fflayer_stack_induce with no iterations is the copy of x, bit for bit"""
    T = backends[dt].T
    rng = np.random.default_rng(3)
    X = np.arange(7 * 13, dtype=dt).reshape(7, 13)
    Y = np.zeros((7, 5), dt)
    Y[:, 0] = 1
    W, b = T.put(rng.standard_normal((5, 13)).astype(dt)), T.put(rng.standard_normal(5).astype(dt))
    y = T.put(Y, batched=True)
    for x in (T.put(X, batched=True), nan_surround(T, X, 7)):
        T.sync()
        before = T.stats()["launches"]
        out, _, _ = T.induce_stack([W], [b], x, y, 0.1, 0)
        launches = T.stats()["launches"] - before
        print("induce, no iterations: launches", launches)
        assert np.array_equal(out.numpy(), X)
        assert launches == 1


# ---- (c) argMax / argMin ----------------------------------------------------------------------------------------------------
def both(T, d, rows):
    """to_arg_max and to_arg_min of handle d against the oracle's fold of `rows` (the rows d holds)"""
    for minimum, f in ((False, T.arg_max), (True, T.arg_min)):
        got = np.atleast_1d(f(d))
        want = RC.arg_reference(rows, minimum)
        bad = np.flatnonzero(got != want)
        assert not len(bad), ("argMin" if minimum else "argMax", rows.shape, bad[:5], got[bad[:5]], want[bad[:5]],
                              rows[bad[0]][:8])


@pytest.mark.parametrize("dt", DTS, ids=IDS)
@pytest.mark.parametrize("n", RC.ARG_NS)
def test_arg_max_min_follow_the_oracle(backends, dt, n):
    T = backends[dt].T
    rows = RC.arg_rows(n, dt)
    K = len(rows)
    for r in rows:                                                   # unbatched
        both(T, T.put(r), r[None])
    for B in RC.ARG_BATCHES + (K,):                                  # batched: B rows of the patterns, every pattern in some batch
        for start in range(0, K, B) if B < 5 else (0, K - min(B, K)):
            sel = rows[(start + np.arange(B)) % K]
            both(T, T.put(sel, batched=True), sel)
    cols = T.transp(T.put(np.ascontiguousarray(rows.T)))             # [K, n] view of a packed [n, K]: row k has stride K
    for k in range(K):
        both(T, T.slice(cols, (k,)), rows[k][None])
    both(T, nan_surround(T, rows, K), rows)                          # a batch_slice view, NaN rows around it
    both(T, nan_surround(T, rows[2], 0), rows[2][None])


def test_arg_max_smallest_nan_case(backends):
    """[1, NaN, 0.5]: the fold takes the NaN, then 0.5 replaces it -- 2, not the 1 that combining lanes in a tree gives"""
    for dt in DTS:
        T = backends[dt].T
        assert T.arg_max(T.put(np.array([1, np.nan, 0.5], dt))) == 2
        assert T.arg_min(T.put(np.array([0.5, np.nan, 1], dt))) == 2
        assert T.arg_max(T.put(np.array([1, 0.5, np.nan], dt))) == 2 and T.arg_max(T.put(np.array([np.nan, 1, 0.5], dt))) == 1


@pytest.mark.parametrize("dt", DTS, ids=IDS)
@pytest.mark.parametrize("nL", [10, 40, 130])
def test_infer_classes_with_nan_columns_follow_the_oracle(backends, dt, nL):
    """to_fflayer_stack_infer (both head kernels): a logistic head with NaN in some columns of every row, NaN in the targets
    too -- classes and the confusion matrix are the oracle's argMax of the stored rows"""
    T = backends[dt].T
    rng = np.random.default_rng(nL)
    B = 70
    X = rng.uniform(-1, 1, (B, 9)).astype(dt)
    Y = rng.integers(-1, 2, (B, nL)).astype(dt)
    Y[rng.integers(0, B, 40), rng.integers(0, nL, 40)] = np.nan
    Y[5, -1] = np.nan
    Y[6] = np.nan
    W1, b1 = (0.5 * rng.standard_normal((6, 9))).astype(dt), (0.5 * rng.standard_normal(6)).astype(dt)
    W2 = (0.5 * rng.standard_normal((nL, 6))).astype(dt)
    for cols in NAN_COLUMNS(nL) + [list(range(nL))]:
        b2 = (0.5 * rng.standard_normal(nL)).astype(dt)
        b2[cols] = np.nan
        out, cls, conf = T.infer_stack([T.put(W1), T.put(W2)], [T.put(b1), T.put(b2)], T.put(X, batched=True), out_act="logistic",
                                       y=T.put(Y, batched=True), want_out=True)
        out = out.numpy()
        assert np.isnan(out[:, cols]).all() and np.isnan(out).sum() == B * len(cols)
        want = RC.arg_reference(out)
        assert np.array_equal(cls, want), (cols, np.flatnonzero(cls != want)[:5])
        assert np.array_equal(cls, T.arg_max(T.put(out, batched=True)))
        wc = np.zeros((nL, nL), np.int64)
        np.add.at(wc, (want, RC.arg_reference(Y)), 1)
        assert np.array_equal(conf, wc), cols
        _, cls2, _ = T.infer_stack([T.put(W1), T.put(W2)], [T.put(b1), T.put(b2)], T.put(X, batched=True), out_act="logistic",
                                   want_out=False)
        assert np.array_equal(cls2, want)           # nothing stored: the row is computed again behind the last NaN


@pytest.mark.parametrize("dt", DTS, ids=IDS)
@pytest.mark.parametrize("route", [0, 2], ids=["per_step", "persistent"])
def test_generate_symbols_with_nan_columns_follow_the_oracle(backends, dt, route):
    """to_rnn_stack_generate, argMax feed, a logistic head with NaN in some columns of every output row: every symbol is the
    oracle's argMax of the stored row before it"""
    from tensor_ops_amd.hipt import HipT
    T = backends[dt].T
    n, B, Tp, G = 70, 5, 2, 5
    rng = np.random.default_rng(70)
    s = T.put((0.1 * rng.standard_normal(6)).astype(dt))
    Ws, W1 = T.put((0.5 * rng.standard_normal((6, 6))).astype(dt)), T.put(rng.standard_normal((6, n)).astype(dt))
    b1, W2 = T.put((0.5 * rng.standard_normal(6)).astype(dt)), T.put(rng.standard_normal((n, 6)).astype(dt))
    X = np.zeros((B, Tp, n), dt)
    X[np.arange(B)[:, None], np.arange(Tp)[None], rng.integers(0, n, (B, Tp))] = 1
    prev = HipT.rnn_generate_persistent(route)
    try:
        for cols in NAN_COLUMNS(n):
            b2 = (0.5 * rng.standard_normal(n)).astype(dt)
            b2[cols] = np.nan
            layers = [(s, Ws, W1, b1, "tanh"), (None, None, W2, T.put(b2))]
            p0 = HipT.rnn_generate_stats()
            out, sym, prime, _ = T.rnn_stack_generate(layers, T.put(X, batched=True), G, "argmax", out_act="logistic",
                                                      want_prime_out=True)
            p1 = HipT.rnn_generate_stats()
            assert (p1[0] - p0[0], p1[1] - p0[1]) == ((1, 0) if route == 2 else (0, 1))
            out, prime = out.numpy(), prime.numpy()
            assert np.isnan(out[:, :, cols]).all() and np.isnan(out).sum() == B * G * len(cols)
            before = np.concatenate([prime[:, -1:], out[:, :-1]], axis=1)      # the stored row each symbol was made from
            for k in range(G):
                assert np.array_equal(sym[:, k], RC.arg_reference(before[:, k])), (cols, k)
    finally:
        HipT.rnn_generate_persistent(prev)


# ---- (d) gather, stack, copy_into_many, broadcasts, oneHot, diag ------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS, ids=IDS)
def test_batch_gather_row_sizes_and_index_counts(backends, dt):
    T = backends[dt].T
    rng = np.random.default_rng(11)
    for numel in RC.gather_numels(dt):
        n_rows = 37
        x = np.arange(n_rows * numel, dtype=dt).reshape(n_rows, numel)
        whole, view = T.put(x, batched=True), nan_surround(T, x, n_rows)   # (the view starts numel elements in: 16-byte aligned only when the row is)
        counts = ("repeated", "reversed") + ((8192, 8193) if numel <= 5 else ())
        for which in counts:
            idx = RC.gather_indices(n_rows, which, rng)
            for d in (whole, view):
                g = T.batch_gather(d, idx)
                assert g.batch == len(idx) and np.array_equal(g.numpy(), x[idx]), (numel, which)
    x = np.arange(40 * 6, dtype=dt).reshape(40, 2, 3)                      # rows of rank 2
    idx = RC.gather_indices(40, "repeated", rng)
    assert np.array_equal(T.batch_gather(nan_surround(T, x, 40), idx).numpy(), x[idx])


@pytest.mark.parametrize("dt", DTS, ids=IDS)
@pytest.mark.parametrize("nrows", RC.STACK_ROWS)
def test_stack_of_rows(backends, dt, nrows):
    T = backends[dt].T
    x = np.arange(nrows * 7, dtype=dt).reshape(nrows, 7)
    assert np.array_equal(T.stack((nrows,), [T.put(r) for r in x]).numpy(), x)            # unbatched rows
    # rows that are slices of one batched tensor: samples bstride = nrows * 7 apart, not numel
    B = 3
    xb = np.arange(B * nrows * 7, dtype=dt).reshape(B, nrows, 7)
    d = T.put(xb, batched=True)
    order = list(range(nrows))[::-1]
    got = T.stack((nrows,), [T.slice(d, (i,)) for i in order])
    assert got.batch == B and np.array_equal(got.numpy(), xb[:, order])
    # strided rows (columns of a matrix) are packed first; a rank-2 lead
    if nrows == 16:
        cols = T.transp(T.put(np.ascontiguousarray(x.T)))
        assert np.array_equal(T.stack((4, 4), [T.slice(cols, (i,)) for i in range(16)]).numpy(), x.reshape(4, 4, 7))


@pytest.mark.parametrize("dt", DTS, ids=IDS)
@pytest.mark.parametrize("pieces,sizes", RC.COPY_MANY)
def test_copy_into_many(backends, dt, pieces, sizes):
    """1, 16 and 17 pieces of whole quads (the 16-byte form, two launches past 16), and one odd piece: the dword form"""
    from tensor_ops_amd import capi
    T = backends[dt].T
    rng = np.random.default_rng(pieces)
    src = [rng.integers(-99, 100, sizes[i % len(sizes)]).astype(dt) for i in range(pieces)]
    ds = [T.put(s) for s in src]
    dd = [T.put(np.full(len(s), 7, dt)) for s in src]
    arr = lambda ts: (capi.c_tensor * len(ts))(*[t.h for t in ts])   # noqa: E731
    T.sync()
    before = T.stats()["launches"]
    capi.check(capi.lib().to_copy_into_many(pieces, arr(dd), arr(ds)))
    assert T.stats()["launches"] - before == (pieces + 15) // 16
    for d, s_, h in zip(dd, ds, src):
        assert np.array_equal(d.numpy(), h) and np.array_equal(s_.numpy(), h)


@pytest.mark.parametrize("dt", DTS, ids=IDS)
def test_map_rows_const_and_batch_bcast(backends, dt):
    T = backends[dt].T
    like_shape = (3, 4, 5)
    like = T.put(np.zeros(like_shape, dt))
    for len_n in (0, 1, 2):
        row = np.arange(int(np.prod(like_shape[len_n:])), dtype=dt).reshape(like_shape[len_n:]) + 1
        got = T.mapRows_const(len_n, T.put(row), like)
        assert got.batch == 0 and np.array_equal(got.numpy(), np.broadcast_to(row, like_shape))
        rb = np.stack([row, row * 2, row * 3 + 1])                         # a batched row under an unbatched shape
        got = T.mapRows_const(len_n, T.put(rb, batched=True), like)
        want = np.stack([np.broadcast_to(r, like_shape) for r in rb])
        assert got.batch == 3 and np.array_equal(got.numpy(), want)
        got = T.mapRows_const(len_n, nan_surround(T, rb, 3), like)         # ... read in place from inside a larger tensor
        assert np.array_equal(got.numpy(), want)
    for shape in ((), (1,), (7,), (3, 5)):
        x = np.arange(int(np.prod(shape)), dtype=dt).reshape(shape) - 2
        for B in (1, 2, 257):
            got = T.batch_bcast(T.put(x), B)
            assert got.batch == B and np.array_equal(got.numpy(), np.broadcast_to(x, (B,) + shape))


@pytest.mark.parametrize("dt", DTS, ids=IDS)
@pytest.mark.parametrize("n,B", RC.ONE_HOT)
def test_one_hot(backends, dt, n, B):
    T = backends[dt].T
    rng = np.random.default_rng(n + B)
    idx = rng.integers(0, n, max(B, 1))
    if B:
        idx[0], idx[-1] = n - 1, 0
    got = T.one_hot(n, 2.5, -0.5, idx if B else int(idx[0]))
    want = np.full((max(B, 1), n), -0.5, dt)
    want[np.arange(max(B, 1)), idx] = 2.5
    assert got.batch == B and np.array_equal(got.numpy(), want if B else want[0])


@pytest.mark.parametrize("dt", DTS, ids=IDS)
@pytest.mark.parametrize("rank,n", RC.DIAG)
def test_diag_and_get_diag(backends, dt, rank, n):
    T = backends[dt].T
    v = np.arange(n, dtype=dt) + 1
    d = T.diag(rank, T.put(v))
    got = d.numpy()
    want = np.zeros((n,) * rank, dt)
    want[tuple([np.arange(n)] * rank)] = v
    assert np.array_equal(got, want)
    assert np.array_equal(T.getDiag(d).numpy(), v)
    x = np.arange(n ** rank, dtype=dt).reshape((n,) * rank)
    assert np.array_equal(T.getDiag(T.put(x)).numpy(), x[tuple([np.arange(n)] * rank)])
    if rank == 2:                                                           # a transposed view: the same diagonal, no pack
        assert np.array_equal(T.getDiag(T.transp(T.put(x))).numpy(), np.diagonal(x))
