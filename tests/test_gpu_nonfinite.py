"""+-inf, NaN and poisoned memory through every contraction route.  Integer sweeps cannot see a kernel that loads a value it
should not have and relies on multiplying it by zero: on finite data `x * 0` vanishes, on +-inf or NaN it becomes a NaN in an
output that IEEE says must be clean.  The reference is tests/nonfinite_ref.py (the class of every output by counting the NaN /
+inf / -inf contributions -- independent of the order of summation, so one reference serves every route; no BLAS is asked about
0 * inf), held against a scalar triple loop by tests/test_nonfinite_ref.py.

 a. the sweeps of test_gpu_fuzz_gemm.py once more with FUZZ_POISON=1 (tools/poison.py): the same shapes, layouts and beta
    choices with poisoned operands, each followed by the clean integer run of the same shape (stale partial tiles)
 b. guard bands: clean operands as views inside a buffer of NaN, at a 16-byte-aligned and at a one-element offset
 c. the gemv family (matVec, vecMat, outerV, sumRows, BLAS gemv / ger, rank-2..15 updates) with the poison IN the operands
 d. the fused epilogues: a recorded `W x + b` alone, under logistic and under tanh; a poisoned bias; beta * C
 e. the per-row calls: a poisoned row stays in its row
 f. a pool whose recycled memory is NaN

Deliberately not IEEE-by-arithmetic, each named where it is expected and nowhere else: beta == 0 does not read
C (the beta-zero tests of c and d); an empty contraction, K = 0, returns zeros without looking at its operands
(test_an_empty_contraction_is_zeros_whatever_surrounds_it); the planner drops the zero tensor `sumT []` from a batch-summed sum
instead of adding B * 0 (test_batch_sum_drops_the_zero_tensor_beside_a_poisoned_term)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import nonfinite_ref as NF
from tools import poison as P

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTS = [np.float32, np.float64]
IDS = ["f32", "f64"]
ACT_TOL = {np.float32: 2e-6, np.float64: 1e-12}      # the project's activation bounds (test_gpu_fuzz_gemm.py, test_gpu_gemv.py)
INF, NAN = np.inf, np.nan


@pytest.fixture(scope="module")
def Ts():
    from tensor_ops_amd.hipt import HipT
    return {np.float32: HipT(0, np.float32), np.float64: HipT(0, np.float64)}


@pytest.fixture(scope="module")
def Bs():
    from tensor_ops_amd.hipb import HipB
    return {np.float32: HipB(0, dtype=np.float32), np.float64: HipB(0, dtype=np.float64)}


def ints(rng, shape, lo=-2, hi=3, dt=np.float32):
    return rng.integers(lo, hi, shape).astype(dt)


def layout(T, x, trans):
    """the matrix x, row-major or as the transposed view of its column-major copy"""
    return T.transp(T.put(np.ascontiguousarray(x.T))) if trans else T.put(x)


def assert_same(got, want, *ctx):
    assert NF.same_class_and_value(got, want), (ctx, NF.describe(got, want))


def assert_act(got, ref, tol, *ctx):
    """NaN exactly where the fp64 reference is NaN; logistic(+-inf) = 1 / 0 and tanh(+-inf) = +-1 are values of the reference"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (ctx, got.shape, ref.shape)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), (ctx, "NaN masks differ", int(np.isnan(got).sum()), int(np.isnan(ref).sum()))
    ok = ~np.isnan(ref)
    err = float(np.max(np.abs(got[ok] - ref[ok]))) if ok.any() else 0.0
    assert err < tol, (ctx, err)


# ---- a. the sweeps, poisoned --------------------------------------------------------------------------------------------------
def _run(tool, *args, env=None):
    try:
        out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", tool)] + [str(a) for a in args], capture_output=True, text=True,
                             timeout=900, env=dict(os.environ, FUZZ_POISON="1", **(env or {})))
    except subprocess.TimeoutExpired as e:      # a hang: nothing more is started on this device before somebody has read the kernel
        pytest.exit("%s %s hung: %s" % (tool, args, str(e.stdout)[-1500:]), returncode=3)
    if out.returncode < 0 or out.returncode in (134, 137, 139):      # ... and the same after an abort or a fault
        pytest.exit("%s %s died with %d: %s" % (tool, args, out.returncode, out.stdout[-1500:] + out.stderr[-1500:]), returncode=3)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "poison " in out.stdout and "skipped 0" in out.stdout, out.stdout[-2000:]
    print(out.stdout[-600:])           # (the coverage line: poisoned cases, how many had non-finite outputs)
    return out.stdout


@pytest.mark.parametrize("cases,seed,env", [(40, 11, {}), (30, 13, {"FUZZ_DTYPE": "f64"})], ids=IDS)
def test_poisoned_random_gemm_extents_and_layouts(cases, seed, env):
    out = _run("gemm_fuzz.py", cases, seed, env=env)
    assert "mismatches 0" in out, out[-3000:]


@pytest.mark.parametrize("dtype,cases", [("f32", 5), ("f64", 3)])
def test_poisoned_large_extents_on_the_pinned_bodies(dtype, cases):
    out = _run("pinned_fuzz.py", cases, 51, env={"FUZZ_DTYPE": dtype})
    assert "mismatches 0" in out, out[-3000:]


def test_poisoned_large_layers_with_bias_and_logistic():
    out = _run("pinned_epilogue_check.py")
    assert "mismatches 0" in out and "MISMATCH" not in out, out[-3000:]


@pytest.mark.parametrize("cases,seed,env", [(10, 43, {"FUZZ_SPLIT": "1"}), (8, 41, {"FUZZ_DTYPE": "f32"}), (8, 41, {"FUZZ_DTYPE": "f64"})],
                         ids=["split", "f32", "f64"])
def test_poisoned_layers_with_fused_epilogues(cases, seed, env):
    out = _run("kw_epilogue_fuzz.py", cases, seed, env=env)
    assert "mismatches 0" in out, out[-3000:]


def test_poisoned_gmul_ranks_and_batches():
    """fp32 and fp64 cases alike (the tool draws the element type per case); one whole sample of a batched operand poisoned too"""
    out = _run("gmul_fuzz.py", 250, 21)
    assert "mismatches 0" in out, out[-3000:]


def test_poisoned_four_wave_32x32_tiles():
    out = _run("t32_check.py")
    assert "t32_check mismatches 0" in out, out[-3000:]


def test_poisoned_tile_menu_kernel():
    out = _run("kw16_check.py", "check")
    assert "kw16_check mismatches 0" in out, out[-3000:]


@pytest.mark.parametrize("env", [{}, {"LEARN_DTYPE": "f64"}], ids=IDS)
def test_poisoned_learn_layer_shapes(env):
    """a tile per wave / per workgroup, K < 128, stream-K over a very long K with up to 64 contributors a tile"""
    shapes = ["8192", "300", "100", "8200", "300", "100", "8192", "100", "300", "100", "8192", "300", "128", "16384", "256", "64", "8192", "784",
              "16", "4096", "2000", "10", "60000", "100", "60000", "100", "12", "300", "784", "6000"]
    out = _run("learn_check.py", *(shapes if not env else shapes[:18]), env=env)
    assert "learn_check mismatches 0" in out, out[-3000:]


@pytest.mark.parametrize("dtype_env,cases,seed", [({}, 100, 21), ({"ROUTE_DTYPE": "f64"}, 60, 22)], ids=IDS)
def test_poisoned_routing_boundaries(dtype_env, cases, seed):
    out = _run("route_fuzz.py", cases, seed, env=dtype_env)
    assert "mismatches 0" in out, out[-3000:]


# ---- b. guard bands ----------------------------------------------------------------------------------------------------------
PAD = 1024      # elements of NaN on either side


def guarded(T, arr, off):
    """arr as a to_wrap view inside a device buffer that is NaN everywhere else, `off` elements beyond a 16-byte boundary;
    (view, base) -- the base tensor has to stay alive as long as the view is used"""
    from tensor_ops_amd import capi
    from tensor_ops_amd.hipt import DT
    dt = T.dtype.type
    host = np.full(PAD + off + arr.size + PAD, NAN, dt)
    host[PAD + off:PAD + off + arr.size] = arr.ravel()
    base = T.put(host)
    assert base.ptr % 16 == 0
    d = (C.c_int64 * max(arr.ndim, 1))(*arr.shape)
    h = capi.c_tensor()
    capi.check(capi.lib().to_wrap(C.c_void_p(base.ptr + (PAD + off) * np.dtype(dt).itemsize), T.to_dtype, arr.ndim, d, 0,
                                  C.byref(h)))
    return DT(h), base


def guarded_layout(T, x, trans, off):
    v, base = guarded(T, np.ascontiguousarray(x.T) if trans else x, off)
    return (T.transp(v) if trans else v), (v, base)


# one per route family (tools/kw16_check.py: the tile menu, ragged; tools/t32_check.py: four waves a 32x32 tile, ragged, a long K;
# tools/learn_check.py: a tile per wave, K < 128, stream-K under a very long K; the pinned body with edge tiles; small / short-K)
GEMM_SHAPES = [(100, 80, 104), (260, 333, 388), (1001, 66, 1003), (480, 83, 496), (1000, 260, 300), (992, 788, 252), (704, 8192, 160),
               (8200, 300, 100), (100, 8192, 300), (10, 6000, 100), (128, 16384, 256), (3001, 290, 3003), (17, 31, 33), (1023, 17, 129)]
RANK_K = [(4096, 8, 4096), (5000, 3, 3000), (2048, 15, 4100), (1000, 7, 4098), (300, 12, 20000), (4097, 2, 1031)]


@pytest.mark.parametrize("dt", DTS, ids=IDS)
@pytest.mark.parametrize("m,k,n", GEMM_SHAPES + RANK_K)
def test_guard_bands_around_gemm_operands(Ts, dt, m, k, n):
    """clean integers surrounded by NaN: a NaN in the product is a read outside an operand's extent that reached an output"""
    T = Ts[dt]
    rng = np.random.default_rng(m + 3 * k + 7 * n)
    a, b = ints(rng, (m, k), dt=dt), ints(rng, (k, n), dt=dt)
    want = a.astype(np.float64) @ b.astype(np.float64)
    for off in (0, 1):
        for ta in (0, 1):
            for tb in (0, 1):
                da, keep_a = guarded_layout(T, a, ta, off)
                db, keep_b = guarded_layout(T, b, tb, off)
                got = T.gmul(1, 1, 1, da, db).numpy()
                assert np.array_equal(got.astype(np.float64), want), (off, ta, tb, NF.describe(got, want))
                del da, db, keep_a, keep_b


@pytest.mark.parametrize("dt", DTS, ids=IDS)
@pytest.mark.parametrize("m,k", [(1536, 4096), (100, 60000), (4099, 515), (257, 8191), (30000, 100), (5000, 2049), (3, 70000), (64, 40000)])
def test_guard_bands_around_matvec_and_vecmat(Ts, dt, m, k):
    T = Ts[dt]
    rng = np.random.default_rng(m * 7 + k)
    A, xk, ym = ints(rng, (m, k), dt=dt), ints(rng, k, dt=dt), ints(rng, m, dt=dt)
    want_mv, want_vm = A.astype(np.float64) @ xk, ym @ A.astype(np.float64)
    for off in (0, 1):
        dx, kx = guarded(T, xk, off)
        dy, ky = guarded(T, ym, off)
        for trans in (0, 1):
            mat, keep = guarded_layout(T, A, trans, off)
            assert np.array_equal(T.matVec(mat, dx).numpy().astype(np.float64), want_mv), (off, trans, "matVec")
            assert np.array_equal(T.vecMat(dy, mat).numpy().astype(np.float64), want_vm), (off, trans, "vecMat")
            assert np.array_equal(T.matVec(T.transp(mat), dy).numpy().astype(np.float64), want_vm), (off, trans, "matVec of the transpose")
            del mat, keep
        del dx, dy, kx, ky


@pytest.mark.parametrize("dt", DTS, ids=IDS)
def test_guard_bands_around_outer_products_and_column_sums(Ts, dt):
    T = Ts[dt]
    rng = np.random.default_rng(77)
    for m, n in ((4096, 784), (1031, 2050), (300, 10000)):
        a, b = ints(rng, m, -3, 4, dt), ints(rng, n, -3, 4, dt)
        for off in (0, 1):
            (da, ka), (db, kb) = guarded(T, a, off), guarded(T, b, off)
            assert np.array_equal(T.outerV(da, db).numpy(), np.outer(a, b)), (m, n, off)
            del da, db, ka, kb
    for m, k in ((60000, 1024), (4096, 4100), (20000, 257), (100001, 10)):
        A = ints(rng, (m, k), dt=dt)
        for off in (0, 1):
            dA, keep = guarded(T, A, off)
            assert np.array_equal(T.sumRows(dA).numpy().astype(np.float64), A.astype(np.float64).sum(axis=0)), (m, k, off)
            del dA, keep


# ---- c. the gemv family, poison in the operands ----------------------------------------------------------------------------
def poisoned_matrix(rng, A, zero_cols=()):
    """the placements of tools/poison.py on one matrix: the first and the last k of a row and the next row's first, the last
    row, the first k beyond the last whole k-tile of 16 and of 32 -- in at most three rows"""
    A = A.copy()
    M, K = A.shape
    m = int(rng.integers(0, max(M - 1, 1)))
    vals = [INF, -INF, NAN]
    pick = lambda: vals[int(rng.integers(3))]
    A[m, 0] = pick(); A[m, K - 1] = pick()
    A[(m + 1) % M, 0] = INF
    A[M - 1, (K // 16) * 16 if K % 16 else max(K - 16, 0)] = pick()
    A[M - 1, (K // 32) * 32 if K % 32 else max(K - 32, 0)] = pick()
    for c in zero_cols:      # an infinity opposite a zero of the vector: NaN is demanded there
        A[m, c] = INF
    return A


GEMV_SHAPES = [(1536, 4096), (100, 60000), (4099, 515), (10000, 300), (257, 8191), (30000, 100), (5000, 2049), (64, 40000), (3, 70000),
               (2048, 2048)]


@pytest.mark.parametrize("dt", DTS, ids=IDS)
@pytest.mark.parametrize("m,k", GEMV_SHAPES)
def test_matvec_and_vecmat_with_poisoned_operands(Ts, dt, m, k):
    T = Ts[dt]
    rng = np.random.default_rng(m * 7 + k + 1)
    A0, xk, ym = ints(rng, (m, k), dt=dt), ints(rng, k, dt=dt), ints(rng, m, dt=dt)
    zc = int(rng.integers(1, k - 1))
    xk[zc] = 0
    A = poisoned_matrix(rng, A0, zero_cols=(zc,))
    want_mv = NF.contract(A, xk[:, None])[:, 0]
    want_vm = NF.contract(ym[None, :], A)[0]
    assert 0 < (~np.isfinite(want_mv)).sum() <= 3 and (~np.isfinite(want_vm)).any() and 2 * np.isfinite(want_vm).sum() > k
    dx, dy = T.put(xk), T.put(ym)
    for trans in (0, 1):
        mat = layout(T, A, trans)
        assert_same(T.matVec(mat, dx).numpy(), want_mv, "matVec", trans)
        assert_same(T.vecMat(dy, mat).numpy(), want_vm, "vecMat", trans)
        assert_same(T.matVec(T.transp(mat), dy).numpy(), want_vm, "matVec of the transpose", trans)
        assert_same(T.vecMat(dx, T.transp(mat)).numpy(), want_mv, "vecMat of the transpose", trans)
    # the poison in the vector: every output whose row meets it is non-finite -- +-inf by the sign of A[m, j], NaN opposite a zero
    xp = xk.copy(); xp[k - 1] = -INF
    want = NF.contract(A0, xp[:, None])[:, 0]
    assert not np.isfinite(want).any()
    for trans in (0, 1):
        assert_same(T.matVec(layout(T, A0, trans), T.put(xp)).numpy(), want, "matVec, vector poisoned", trans)
    # the clean operands once more (partial sums of a split reduction come from the pool)
    assert np.array_equal(T.matVec(T.put(A0), dx).numpy().astype(np.float64), A0.astype(np.float64) @ xk)


@pytest.mark.parametrize("dt", DTS, ids=IDS)
@pytest.mark.parametrize("m,n", [(4096, 784), (1031, 2050), (10000, 300), (300, 10000), (2048, 2048), (60000, 100)])
def test_outer_products_with_poisoned_operands(Ts, Bs, dt, m, n):
    T = Ts[dt]
    rng = np.random.default_rng(m + 3 * n + 1)
    a0, b0 = ints(rng, m, -3, 4, dt), ints(rng, n, -3, 4, dt)
    for kind in P.KINDS:
        a, b = P.pair(a0[:, None], b0[None, :], kind=kind, rng=rng)
        want = NF.contract(a, b)
        P.check_case(want, m, n)
        assert_same(T.outerV(T.put(a[:, 0]), T.put(b[0])).numpy(), want, "outerV", kind)
        assert_same(Bs[dt].ger(T.put(a[:, 0]), T.put(b[0])).numpy(), want, "ger", kind)


@pytest.mark.parametrize("dt", DTS, ids=IDS)
@pytest.mark.parametrize("m,k", [(60000, 1024), (10000, 10000), (4096, 4100), (20000, 257), (1000000, 10)])
def test_tall_column_sums_with_poisoned_entries(Ts, dt, m, k):
    T = Ts[dt]
    rng = np.random.default_rng(m + k + 1)
    A = ints(rng, (m, k), dt=dt)
    A[0, 0] = INF                                     # one infinity: that infinity
    A[m - 1, 1] = -INF; A[m // 2, 1] = -INF           # the same sign twice: still that infinity
    A[1, 2] = INF; A[m - 1, 2] = -INF                 # both signs in one column: NaN
    A[m - 1, k - 1] = NAN                             # the last element of the matrix
    A[int(rng.integers(m)), k // 2] = NAN
    want = NF.sum_rows(A)
    assert want[0] == INF and want[1] == -INF and np.isnan(want[2]) and np.isnan(want[k - 1]) and np.isfinite(want).sum() == k - 5
    assert_same(T.sumRows(T.put(A)).numpy(), want)


@pytest.mark.parametrize("dt", DTS, ids=IDS)
def test_blas_gemv_with_beta_y_and_poison(Bs, dt):
    B = Bs[dt]
    rng = np.random.default_rng(6)
    for m, k in ((3000, 4100), (100, 50000), (20000, 120)):
        A0, x, y = ints(rng, (m, k), dt=dt), ints(rng, k, dt=dt), ints(rng, m, -4, 5, dt)
        A = poisoned_matrix(rng, A0)
        yp = y.copy(); yp[m // 3] = INF; yp[m // 3 + 1] = NAN
        dA, dx = B.T.put(A), B.T.put(x)
        want = NF.contract_epilogue(A, x[:, None], 2.0, -3.0, yp[:, None])[:, 0]
        assert want[m // 3] == -INF or np.isnan(want[m // 3])
        assert_same(B.gemv(2.0, dA, dx, (-3.0, B.T.put(yp))).numpy(), want, (m, k), "beta y")
        assert_same(B.gemv(1.0, dA, dx, None).numpy(), NF.contract(A, x[:, None])[:, 0], (m, k))
        # beta == 0 does not read y (the BLAS convention; deliberately not IEEE: 0 * NaN would be NaN)
        got = B.gemv(1.0, B.T.put(A0), dx, (0.0, B.T.put(yp))).numpy()
        assert np.array_equal(got.astype(np.float64), A0.astype(np.float64) @ x), (m, k, "beta == 0")


@pytest.mark.parametrize("dt", DTS, ids=IDS)
@pytest.mark.parametrize("m,k,n", [(4096, 8, 4096), (5000, 3, 3000), (2048, 15, 4100), (1000, 7, 4098), (60000, 8, 256), (300, 12, 20000),
                                   (4096, 2, 1030), (2050, 7, 4100)])      # (1000 x 7 x 4098 is below the kernel's 4M outputs: another route)
def test_rank_k_updates_with_poisoned_operands(Ts, Bs, dt, m, k, n):
    """gemv.hip's outer-product kernel keeps the rank rounded up to 8 or 16 in registers.  Beyond K it used to reload a[m][0]
    and multiply it by a zeroed row of b: with a[m][0] = +inf every output of row m came back NaN (inf + inf * 0) where +-inf (or,
    opposite a zero of b, NaN) is the IEEE value -- on every K other than 1, 8 and 16, in both element types."""
    T, B = Ts[dt], Bs[dt]
    rng = np.random.default_rng(m + 5 * k + n + 1)
    a0, b0, c = ints(rng, (m, k), dt=dt), ints(rng, (k, n), dt=dt), ints(rng, (m, n), -5, 6, dt)
    # the issue's case: +inf at a[m][0]; rows of b without a zero in row 0 would do, a random row has both
    a = a0.copy(); r = m // 2
    a[r, 0] = INF
    want = NF.contract(a, b0)
    assert (want[r] == INF).any() and (want[r] == -INF).any() and np.isnan(want[r]).any() and np.isfinite(np.delete(want, r, axis=0)).all()
    for ta in (0, 1):
        for tb in (0, 1):
            got = T.gmul(1, 1, 1, layout(T, a, ta), layout(T, b0, tb)).numpy()
            print("rank-%d update %d x %d, +inf at a[%d][0], ta %d tb %d: row %d holds %d NaN where the reference holds %d (and %d infinities)"
                  % (k, m, n, r, ta, tb, r, int(np.isnan(got[r]).sum()), int(np.isnan(want[r]).sum()), int(np.isinf(want[r]).sum())))
            assert_same(got, want, "inf at a[m][0]", ta, tb)
    for kind in P.KINDS:
        ap, bp = P.pair(a0, b0, kind=kind, rng=rng)
        want = NF.contract(ap, bp)
        P.check_case(want, m, n)
        ta, tb = int(rng.integers(2)), int(rng.integers(2))
        assert_same(T.gmul(1, 1, 1, layout(T, ap, ta), layout(T, bp, tb)).numpy(), want, kind, ta, tb)
    # `gemm alpha a b (Just (beta, c))`: the poison in a, in c, and -- under beta == 0 -- in a c that must not be read
    cp = c.copy(); cp[1, 1] = NAN; cp[m - 1, n - 1] = -INF; cp[2, 0] = INF
    got = B.gemm(2.0, T.put(a), T.put(b0), (-3.0, T.put(cp))).numpy()
    assert_same(got, NF.contract_epilogue(a, b0, 2.0, -3.0, cp), "gemm, beta c")
    got = B.gemm(2.0, T.put(a0), T.put(b0), (0.0, T.put(cp))).numpy()
    assert np.array_equal(got.astype(np.float64), 2.0 * (a0.astype(np.float64) @ b0.astype(np.float64))), "beta == 0 read c"


# ---- d. fused epilogues ----------------------------------------------------------------------------------------------------
def recorded_layer(T, dW, dX, db, o, act, key):
    from tensor_ops_amd import hipt
    with T.memo():
        z = T.sumT([T.matVec(dW, dX), db], (o,))
        if act == "logistic":
            z = T.liftT(hipt.logistic_closure, [z], key=key + "-logistic")
        elif act == "tanh":
            z = T.liftT(lambda v: hipt.tanh(v[0]), [z], key=key + "-tanh")
        return T.force(z).numpy()


def check_layer(T, dt, X, W, b, ctx):
    """z = X W^T + b exactly (class and value); logistic(z), tanh(z) within the activation bounds of fp64 numpy, NaN where it is NaN"""
    M, o = X.shape[0], W.shape[0]
    want = NF.contract_epilogue(X, W.T, bias=b)
    dW, dX, db = T.put(W), T.put(X, batched=True), T.put(b)
    assert_same(recorded_layer(T, dW, dX, db, o, None, "nf").reshape(M, o), want.astype(dt), ctx, "W x + b")
    assert_act(recorded_layer(T, dW, dX, db, o, "logistic", "nf").reshape(M, o), P.logistic(want), ACT_TOL[dt], ctx, "logistic")
    assert_act(recorded_layer(T, dW, dX, db, o, "tanh", "nf").reshape(M, o), np.tanh(want), 10 * ACT_TOL[dt], ctx, "tanh")
    return want


# (M, K, N): tools/pinned_epilogue_check.py (the pinned body: whole tiles, edge tiles, a short K), tools/kw_epilogue_fuzz.py's
# ranges (mid-size, and few tiles under a long K), the training step's layers (test_gpu_step_overlap.py: 1024 x 784 x 256,
# 1024 x 256 x 10)
LAYER_SHAPES = [(4096, 64, 4096), (4000, 288, 4000), (8192, 48, 2048), (1500, 500, 700), (2599, 899, 131), (700, 3000, 300), (1024, 784, 256),
                (1024, 256, 10)]


@pytest.mark.parametrize("dt", DTS, ids=IDS)
@pytest.mark.parametrize("M,K,N", LAYER_SHAPES)
def test_fused_epilogues_with_poison(Ts, dt, M, K, N):
    if dt is np.float64 and M * N > 4096 * 2048:
        M, N = M // 2, N // 2          # (the fp64 sweeps of tools/kw_epilogue_fuzz.py stay below 1400 x 700 too)
    T = Ts[dt]
    rng = np.random.default_rng(M + K + N)
    W0, X0, b0 = ints(rng, (N, K), dt=dt), ints(rng, (M, K), dt=dt), ints(rng, N, -3, 4, dt)
    for kind in P.KINDS[:2] if M * N > 4e6 else P.KINDS:
        X, Wt = P.pair(X0, W0.T, kind=kind, rng=rng)
        want = check_layer(T, dt, X, np.ascontiguousarray(Wt.T), b0, kind)
        P.check_case(want, M, N)
    # a poisoned bias: its columns are +inf -> 1 / 1, -inf -> 0 / -1, NaN -> NaN in every row; everything else as before
    b = b0.copy(); b[0] = INF; b[N - 1] = -INF; b[N // 2] = NAN
    want = check_layer(T, dt, X0, W0, b, "bias")
    assert (want[:, 0] == INF).all() and (want[:, N - 1] == -INF).all() and np.isnan(want[:, N // 2]).all()
    # ... and meeting the opposite infinity of the product: NaN
    X = X0.copy(); X[3, 0] = INF
    W = W0.copy(); W[0, 0] = -1; W[N - 1, 0] = -1
    want = check_layer(T, dt, X, W, b, "bias against the product")
    assert np.isnan(want[3, 0]) and want[3, N - 1] == -INF


@pytest.mark.parametrize("dt", DTS, ids=IDS)
@pytest.mark.parametrize("i,o", [(4096, 4096), (60000, 300), (300, 60000)])
def test_a_wide_layer_on_one_sample_with_poison(Ts, dt, i, o):
    """`logistic (W x + b)` for ONE sample (gemv.hip's epilogue; a split reduction has a finishing pass)"""
    from tensor_ops_amd import hipt
    T = Ts[dt]
    rng = np.random.default_rng(i + o + 1)
    W0 = (rng.integers(-2, 3, (o, i)) / 64).astype(dt); x = ints(rng, i, dt=dt); b = (rng.integers(-3, 4, o) / 8).astype(dt)
    zc = int(rng.integers(1, i - 1)); x[zc] = 0
    W = poisoned_matrix(rng, W0, zero_cols=(zc,))
    b[o - 2] = INF; b[1] = NAN
    z = NF.contract_epilogue(x[None, :], W.T, bias=b)[0]
    assert 3 <= (~np.isfinite(z)).sum() <= 5
    dW, dx, db = T.put(W), T.put(x), T.put(b)
    with T.memo():
        pre = T.force(T.sumT([T.matVec(dW, dx), db], (o,))).numpy()
    # (the weights are multiples of 1/64 and the bias of 1/8: the finite sums are exact in both element types)
    assert_same(pre, z.astype(dt), "W x + b")
    with T.memo():
        out = T.force(T.liftT(hipt.logistic_closure, [T.sumT([T.matVec(dW, dx), db], (o,))], key="gemv-logistic")).numpy()
    assert_act(out, P.logistic(z), ACT_TOL[dt], "logistic")
    with T.memo():
        out = T.force(T.liftT(lambda v: hipt.tanh(v[0]), [T.sumT([T.matVec(dW, dx), db], (o,))], key="gemv-tanh")).numpy()
    assert_act(out, np.tanh(z), 10 * ACT_TOL[dt], "tanh")


@pytest.mark.parametrize("dt", DTS, ids=IDS)
@pytest.mark.parametrize("m,k,n", [(1000, 260, 300), (128, 16384, 256), (2048, 512, 2048), (100, 80, 104), (4000, 288, 4000), (704, 8192, 160)])
def test_beta_c_with_poison_and_beta_zero_without(Ts, Bs, dt, m, k, n):
    """`gemm alpha a b (Just (beta, c))`: a poisoned c reaches exactly its own elements under beta != 0, and nothing under beta == 0
    -- the BLAS convention (the kernels test `beta != 0.0`), deliberately not IEEE, expected here and nowhere else"""
    T, B = Ts[dt], Bs[dt]
    rng = np.random.default_rng(m + k + n + 2)
    a0, b0, c0 = ints(rng, (m, k), dt=dt), ints(rng, (k, n), dt=dt), ints(rng, (m, n), -4, 5, dt)
    c = c0.copy(); c[0, 0] = NAN; c[m - 1, n - 1] = INF; c[m // 2, :] = -INF; c[5, n - 1] = INF
    a, b = P.pair(a0, b0, kind="k-ends", rng=rng)
    for ta, tb in ((0, 0), (1, 1), (0, 1)):
        da, db = layout(T, a0, ta), layout(T, b0, tb)
        got = B.gemm(-2.0, da, db, (3.0, T.put(c))).numpy()
        assert_same(got, NF.contract_epilogue(a0, b0, -2.0, 3.0, c), "clean product, poisoned c", ta, tb)
        got = B.gemm(-2.0, layout(T, a, ta), layout(T, b, tb), (3.0, T.put(c))).numpy()
        assert_same(got, NF.contract_epilogue(a, b, -2.0, 3.0, c), "poisoned product, poisoned c", ta, tb)
        got = B.gemm(-2.0, da, db, (0.0, T.put(c))).numpy()
        assert np.array_equal(got.astype(np.float64), -2.0 * (a0.astype(np.float64) @ b0.astype(np.float64))), ("beta == 0 read c", ta, tb)


# ---- e. a poisoned row stays in its row --------------------------------------------------------------------------------------
def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def nn_weights(rng, sizes, dt, scale=0.5):
    return [((scale * rng.standard_normal((o, i))).astype(dt), (scale * rng.standard_normal(o)).astype(dt)) for i, o in zip(sizes[:-1], sizes[1:])]


def forward64(ws, X, head):
    """tests/test_gpu_infer.py's fp64 forward"""
    a = X.astype(np.float64)
    with np.errstate(all="ignore"):
        for l, (w, b) in enumerate(ws):
            z = a @ w.astype(np.float64).T + b.astype(np.float64)
            if l + 1 < len(ws) or head == "logistic":
                a = 1 / (1 + np.exp(-z))
            else:
                e = np.exp(z - z.max(axis=1, keepdims=True))
                a = e / e.sum(axis=1, keepdims=True)
    return a


@pytest.mark.parametrize("dt", DTS, ids=IDS)
@pytest.mark.parametrize("sizes,B", [([784, 300, 100, 10], 4001), ([100, 10], 3000), ([13, 9, 40], 65), ([4097, 32], 300)])
@pytest.mark.parametrize("head", ["softmax", "logistic"])
def test_infer_stack_keeps_a_poisoned_row_to_itself(Ts, dt, sizes, B, head):
    T = Ts[dt]
    rng = np.random.default_rng(B + sizes[0])
    ws = nn_weights(rng, sizes, dt, scale=0.1 if sizes[0] > 100 else 0.5)
    X = rng.uniform(-1, 1, (B, sizes[0])).astype(dt)
    Y = np.zeros((B, sizes[-1]), dt); Y[np.arange(B), rng.integers(0, sizes[-1], B)] = 1
    W, b = [T.put(w) for w, _ in ws], [T.put(bb) for _, bb in ws]
    y = T.put(Y, batched=True)
    clean, _, conf0 = T.infer_stack(W, b, T.put(X, batched=True), out_act=head, y=y, want_out=True)
    clean = clean.numpy()
    tol = {np.float32: 1e-5, np.float64: 1e-12}[dt]     # (test_gpu_infer.py's)
    for row, col, v in ((B // 2, 0, NAN), (B - 1, sizes[0] - 1, INF), (0, sizes[0] // 2, NAN)):
        Xp = X.copy(); Xp[row, col] = v
        out, cls, conf = T.infer_stack(W, b, T.put(Xp, batched=True), out_act=head, y=y, want_out=True)
        out = out.numpy()
        ref = forward64(ws, Xp, head)
        # the poisoned row: NaN exactly where the fp64 forward is NaN (an infinity can saturate a logistic into a finite
        # row), and the reference's value within the tolerance everywhere else
        assert np.isnan(ref[row]).all() or v == INF, (row, col, v)
        print("infer_stack %s %s row %d, %r at column %d: %d of %d reference outputs NaN" % (sizes, head, row, v, col, int(np.isnan(ref[row]).sum()), ref.shape[1]))
        assert np.array_equal(np.isnan(out[row]), np.isnan(ref[row])), (row, col, v, out[row], ref[row])
        fin = ~np.isnan(ref[row])
        assert not fin.any() or np.abs(out[row][fin] - ref[row][fin]).max() <= tol, (row, col, v)
        others = np.arange(B) != row
        assert np.array_equal(bits(out[others]), bits(clean[others])), (row, col, v)
        assert np.abs(out[others] - ref[others]).max() <= tol
        assert conf.sum() == B and conf0.sum() == B


@pytest.mark.parametrize("dt", DTS, ids=IDS)
@pytest.mark.parametrize("B,i,o", [(1024, 784, 256), (4001, 300, 100), (301, 4097, 32), (8192, 48, 2048)])
def test_a_batched_forward_layer_keeps_a_poisoned_row_to_itself(Ts, dt, B, i, o):
    T = Ts[dt]
    rng = np.random.default_rng(B + i + o)
    W, bb = (0.1 * rng.standard_normal((o, i))).astype(dt), (0.1 * rng.standard_normal(o)).astype(dt)
    X = rng.uniform(-1, 1, (B, i)).astype(dt)
    dW, db = T.put(W), T.put(bb)
    clean = recorded_layer(T, dW, T.put(X, batched=True), db, o, "logistic", "nf-row").reshape(B, o)
    for row, col, v in ((B // 2, 0, NAN), (B - 1, i - 1, NAN), (0, (i // 32) * 32 if i % 32 else i - 32, NAN)):
        Xp = X.copy(); Xp[row, col] = v
        out = recorded_layer(T, dW, T.put(Xp, batched=True), db, o, "logistic", "nf-row").reshape(B, o)
        assert np.isnan(out[row]).all(), (row, col)
        others = np.arange(B) != row
        assert np.array_equal(bits(out[others]), bits(clean[others])), (row, col)
        with np.errstate(all="ignore"):
            ref = 1 / (1 + np.exp(-(X.astype(np.float64) @ W.astype(np.float64).T + bb)))
        assert np.abs(out[others] - ref[others]).max() <= {np.float32: 1e-5, np.float64: 1e-12}[dt]


@pytest.mark.parametrize("mode", [0, 2], ids=["per-step", "persistent"])
@pytest.mark.parametrize("dt", DTS, ids=IDS)
def test_rnn_stack_run_keeps_a_poisoned_sequence_to_itself(Ts, dt, mode):
    import rnn_numpy as RN
    from tensor_ops_amd.hipt import HipT
    T = Ts[dt]
    rng = np.random.default_rng(12)
    layers, prev = [], 6
    for n, st in [(48, True), (20, True), (7, False)]:      # (test_gpu_rnn_stack.py's stack of the batch-independence test)
        Wm, b = 0.5 * rng.standard_normal((n, prev)), 0.5 * rng.standard_normal(n)
        s, ws = (0.5 * rng.standard_normal(n), 0.5 * rng.standard_normal((n, n))) if st else (None, None)
        layers.append(tuple(None if v is None else np.asarray(v, dt) for v in (s, ws, Wm, b)))
        prev = n
    dl = [tuple(None if v is None else T.put(v) for v in lay) for lay in layers]
    B, steps = 9, 12
    X = rng.uniform(-1, 1, (B, steps, 6)).astype(dt)
    prev_mode = HipT.rnn_persistent(mode)
    try:
        clean = T.rnn_stack_run(dl, T.put(X, batched=True), "softmax")[0].numpy()
        for row, t in ((4, 0), (8, 5), (0, steps - 1)):
            Xp = X.copy(); Xp[row, t, 2] = NAN
            out = T.rnn_stack_run(dl, T.put(Xp, batched=True), "softmax")[0].numpy()
            with np.errstate(all="ignore"):
                ref = RN.forward(layers, Xp.astype(np.float64), "softmax")[0]
            assert np.isnan(ref[row, t:]).all() and not np.isnan(ref[row, :t]).any()
            assert np.isnan(out[row][np.isnan(ref[row])]).all(), (row, t)
            others = np.arange(B) != row
            assert np.array_equal(bits(out[others]), bits(clean[others])), (row, t)
            assert np.array_equal(bits(out[row, :t]), bits(clean[row, :t])), (row, t)      # (and the steps before the poison)
            err = np.linalg.norm((out[others] - ref[others]).ravel()) / np.linalg.norm(ref[others].ravel())
            assert err < {np.float32: 1e-5, np.float64: 1e-11}[dt]      # (test_gpu_rnn_stack.py's)
    finally:
        HipT.rnn_persistent(prev_mode)


@pytest.mark.parametrize("mode", [0, 2], ids=["per-iteration", "persistent"])
@pytest.mark.parametrize("dt", DTS, ids=IDS)
def test_induce_stack_keeps_a_poisoned_row_to_itself(Ts, dt, mode):
    """[7, 12, 8, 10] fits one workgroup's plan (tests/test_gpu_induce.py): forcing the persistent route there is in range"""
    import induce_numpy as IN
    T = Ts[dt]
    sizes, B = [7, 12, 8, 10], 37
    rng = np.random.default_rng(3)
    ws = nn_weights(rng, sizes, dt)
    X = rng.uniform(-1, 1, (B, sizes[0])).astype(dt)
    Y = np.zeros((B, sizes[-1]), dt); Y[np.arange(B), rng.integers(0, sizes[-1], B)] = 1
    W, b = [T.put(w) for w, _ in ws], [T.put(bb) for _, bb in ws]
    y = T.put(Y, batched=True)
    prev_mode = T.induce_persistent(mode)
    try:
        p0, q0 = T.induce_stats()
        clean = T.induce_stack(W, b, T.put(X, batched=True), y, 0.3, 6)[0].numpy()
        p1, q1 = T.induce_stats()
        assert (p1 - p0, q1 - q0) == ((1, 0) if mode == 2 else (0, 1))      # (the route asked for is the route that ran)
        for row, col in ((17, 0), (36, 6), (0, 3)):
            Xp = X.copy(); Xp[row, col] = NAN
            out = T.induce_stack(W, b, T.put(Xp, batched=True), y, 0.3, 6)[0].numpy()
            with np.errstate(all="ignore"):
                ref = IN.induce(ws, Xp, Y, 0.3, 6)[0]
            assert np.isnan(ref[row]).any() and np.isnan(out[row][np.isnan(ref[row])]).all(), (row, col)
            others = np.arange(B) != row
            assert np.array_equal(bits(out[others]), bits(clean[others])), (row, col)
            assert np.abs(out[others].astype(np.float64) - ref[others]).max() <= {np.float32: 1e-5, np.float64: 1e-12}[dt]
    finally:
        T.induce_persistent(prev_mode)


# ---- the two other deliberate non-IEEE-by-arithmetic behaviours ---------------------------------------
@pytest.mark.parametrize("dt", DTS, ids=IDS)
def test_an_empty_contraction_is_zeros_whatever_surrounds_it(Ts, nan_pool, dt):
    """K = 0: the empty sum is zero, and it is produced without looking at the operands -- an M x 0 and a 0 x N operand own no
    element, so the poison is all around them instead: the views lie inside a buffer of NaN (what any load through their pointers
    would fetch) and the result comes out of a pool whose recycled memory is NaN (an output left unwritten would show it).  The
    narrow expectation: every output is exactly zero; nothing else about K = 0 is asserted."""
    T = Ts[dt]
    for m, n in ((300, 70), (1, 1), (4097, 33), (7, 5000)):
        for off in (0, 1):
            for ta in (0, 1):
                for tb in (0, 1):
                    da, keep_a = guarded_layout(T, np.zeros((m, 0), dt), ta, off)
                    db, keep_b = guarded_layout(T, np.zeros((0, n), dt), tb, off)
                    nan_pool()
                    got = T.gmul(1, 1, 1, da, db).numpy()
                    assert got.shape == (m, n) and np.array_equal(got, np.zeros((m, n), dt)), (m, n, off, ta, tb, NF.describe(got, np.zeros((m, n))))
                    del da, db, keep_a, keep_b
    # ... the same under the batch-summed form with a batch of empty contractions
    a, b = T.put(np.zeros((5, 12, 0), dt), batched=True), T.put(np.zeros((5, 0, 9), dt), batched=True)
    nan_pool()
    got = T.gmul_batch_sum(1, 1, 1, a, b).numpy()
    assert got.shape == (12, 9) and np.array_equal(got, np.zeros((12, 9), dt))


@pytest.mark.parametrize("dt", DTS, ids=IDS)
@pytest.mark.parametrize("B,n", [(33, 300), (5, 4099), (1024, 10)])
def test_batch_sum_drops_the_zero_tensor_beside_a_poisoned_term(Ts, dt, B, n):
    """sum_b (x_b + 0): the planner drops the unbatched zero tensor `sumT []` instead of adding B * 0.  Beside a poisoned x that
    is visible in nothing but the sign of a zero (which no comparison here looks at): the infinities and NaN of x reach exactly
    their own columns, every other column is the integer sum.  The narrow expectation: recorded and eager, the result is the
    class and value of sum_b x_b alone."""
    T = Ts[dt]
    rng = np.random.default_rng(B + n)
    x = ints(rng, (B, n), dt=dt)
    x[:, 6] = 0; x[1, 6] = 1; x[2, 6] = -1               # a column whose sum is an exact zero
    x[3, 0] = INF; x[B - 1, 0] = INF                      # one sign twice: that infinity
    x[0, 1] = INF; x[4, 1] = -INF                         # both signs: NaN
    x[B - 1, n - 1] = NAN; x[2, 2] = -INF
    want = NF.sum_rows(x)
    assert want[0] == INF and np.isnan(want[1]) and want[2] == -INF and np.isnan(want[n - 1]) and want[6] == 0 and np.isfinite(want).sum() == n - 4
    with T.memo():
        z = T.sumT([T.put(x, batched=True), T.sumT([], (n,))], (n,))
        got = T.force(T.batch_sum(z)).numpy()
    assert_same(got, want.astype(dt), "recorded")
    with T.memo():      # the zero tensor first, and between two batched terms
        dx = T.put(x, batched=True)
        z = T.sumT([T.sumT([], (n,)), dx, T.sumT([], (n,)), dx], (n,))
        got = T.force(T.batch_sum(z)).numpy()
    assert_same(got, NF.sum_rows(np.concatenate([x, x])).astype(dt), "recorded, twice")
    got = T.batch_sum(T.sumT([T.put(x, batched=True), T.sumT([], (n,))], (n,))).numpy()
    assert_same(got, want.astype(dt), "eager")


# ---- f. a recycled pool -------------------------------------------------------------------------------------------------------
@pytest.fixture
def nan_pool(Ts):
    """Upload and release NaN-filled tensors of assorted sizes: the pool memory handed out next -- every result, and the partial
    sums of gemv.hip's split reductions -- is NaN.  The partial-tile workspace of the split-K, stream-K and wave-split GEMM forms
    is NOT pool memory: it is one process-wide allocation made at to_init (gemm_kwave.hip), as are the arrival counters of
    gemm_t32.hip, gemm_kwave.hip and gemm_small.hip (zeroed there).  What a recycled pool cannot reach in that workspace, the
    clean-after-poison reruns cover: below, and in every FUZZ_POISON sweep, the clean product follows the poisoned one."""
    def fill():
        for T in Ts.values():
            held = [T.put(np.full(n, NAN, T.dtype.type)) for n in (7, 256, 4096, 65536, 1 << 20, 3 << 20, 1 << 24, (1 << 25) + 5, 1 << 26)]
            T.sync()
            del held
    fill()
    return fill


@pytest.mark.parametrize("dt", DTS, ids=IDS)
def test_products_out_of_a_pool_of_nan(Ts, Bs, nan_pool, dt):
    T = Ts[dt]
    rng = np.random.default_rng(99)
    # split-K with a workspace and a second pass, stream-K, the wave-split kernels' partial tiles, a tile per wave, short K
    for m, k, n in ((1024, 1024, 1024), (2048, 2048, 2048), (128, 16384, 256), (704, 8192, 160), (1280, 4096, 1280), (3, 70000, 1), (100, 60000, 1),
                    (4352, 1024, 4352), (1000, 7, 4098)):
        a0, b0 = ints(rng, (m, k), dt=dt), ints(rng, (k, n), dt=dt)
        a, b = P.pair(a0, b0, rng=rng)
        nan_pool()
        assert_same(T.gmul(1, 1, 1, T.put(a), T.put(b)).numpy(), NF.contract(a, b), (m, k, n), "poisoned")
        nan_pool()
        got = T.gmul(1, 1, 1, T.put(a0), T.put(b0)).numpy()
        assert np.array_equal(got.astype(np.float64), a0.astype(np.float64) @ b0.astype(np.float64)), (m, k, n, NF.describe(got, a0.astype(np.float64) @ b0.astype(np.float64)))
    for M, K, N in ((700, 3000, 300), (1024, 784, 256)):
        W0, X0, b0 = ints(rng, (N, K), dt=dt), ints(rng, (M, K), dt=dt), ints(rng, N, -3, 4, dt)
        nan_pool()
        check_layer(T, dt, X0, W0, b0, "clean layer out of a pool of NaN")
        X, Wt = P.pair(X0, W0.T, rng=rng)
        nan_pool()
        check_layer(T, dt, X, np.ascontiguousarray(Wt.T), b0, "poisoned layer out of a pool of NaN")
