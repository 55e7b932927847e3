"""The split-bf16 fp32 GEMM (csrc/gemm_split.hip; `to_set_gemm_f32_split`) forced with six and nine products against a plain
`np.longdouble` product: bit-exact where every partial sum is exact, plane by plane, in all four layouts; every epilogue at the
fp32 bar; non-finite operands; the switch.  Every test puts the previous mode back."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FAM = "split"
F32 = np.float32
LAYOUTS = [(0, 0), (0, 1), (1, 0), (1, 1)]
PRODUCTS = [6, 9]
# (m, k, n): one 32 x 32 x 16 MFMA block; ragged everything; one past the 256 x 128 tile in M and in N with a K of one 16-deep
# k-tile + 6; two k-tiles exactly.  K <= 254 keeps every partial sum exact: in units of 2^-16 a term is at most 66049
EXACT_SHAPES = [(32, 16, 32), (37, 150, 70), (257, 22, 129), (64, 32, 64)]
EPI_SHAPES = [(37, 150, 70), (257, 40, 129)]


@pytest.fixture(scope="module")
def T():
    from tensor_ops_amd.hipt import HipT
    return HipT(0, dtype=F32)


@pytest.fixture()
def split(T):
    first = []

    def set_(mode, products=-1):
        first.append(T.set_gemm_f32_split(mode, products))
    yield set_
    if first:
        T.set_gemm_f32_split(first[0])


def ld(x):
    return x.astype(np.longdouble)


def row_err(got, want):
    return float(np.max(np.max(np.abs(got - want), axis=1) / np.max(np.abs(want), axis=1)))


def exact_data(kind, rng, m, k, n):
    """ints: one piece.  mid: i + j 2^-8 on both sides (a0 b1, a1 b0, a1 b1).  low_a / low_b: s (1 + 2^-8 + j 2^-16), s in {-1, 0, 1},
    j in {0, 1} -- truncated into 1, 2^-8 and 2^-16, a non-zero THIRD piece where j = 1 -- against {-1, 0, 1} (a2 b0 / a0 b2)"""
    low = lambda shape: t(shape) * (1 + 2.0 ** -8 + rng.integers(0, 2, size=shape) * 2.0 ** -16)   # noqa: E731
    t = lambda shape: rng.integers(-1, 2, size=shape).astype(np.float64)   # noqa: E731
    if kind == "ints":
        a, b = rng.integers(-3, 4, size=(m, k)), rng.integers(-3, 4, size=(k, n))
    elif kind == "mid":
        a, b = t((m, k)) + t((m, k)) * 2.0 ** -8, t((k, n)) + t((k, n)) * 2.0 ** -8
    elif kind == "low_a":
        a, b = low((m, k)), t((k, n))
    else:
        a, b = t((m, k)), low((k, n))
    return a.astype(F32), b.astype(F32)


@pytest.mark.parametrize("ta,tb", LAYOUTS)
@pytest.mark.parametrize("products", PRODUCTS)
@pytest.mark.parametrize("kind", ["ints", "mid", "low_a", "low_b"])
@pytest.mark.parametrize("mkn", EXACT_SHAPES, ids=["%dx%dx%d" % s for s in EXACT_SHAPES])
def test_forced_is_bit_exact_where_every_sum_is(T, split, mkn, kind, products, ta, tb):
    (m, k, n), (a, b) = mkn, exact_data(kind, np.random.default_rng(7300 + 2 * ta + tb), *mkn)
    split(2, products)
    assert T.gemm_route(m, k, n, "f32", a_transposed=bool(ta), b_transposed=bool(tb))["families"] == [FAM]
    da = T.transp(T.put(np.ascontiguousarray(a.T))) if ta else T.put(a)
    db = T.transp(T.put(np.ascontiguousarray(b.T))) if tb else T.put(b)
    st = T.stats()["launches"]
    got = T.gmul(1, 1, 1, da, db)
    assert T.stats()["launches"] - st == 2       # the split pre-pass and the product
    assert np.array_equal(got.numpy(), (ld(a) @ ld(b)).astype(F32))


@pytest.mark.parametrize("products", PRODUCTS)
@pytest.mark.parametrize("epi", ["plain", "alpha", "beta", "alias", "logistic", "tanh"])
@pytest.mark.parametrize("mkn", EPI_SHAPES, ids=["%dx%dx%d" % s for s in EPI_SHAPES])
def test_epilogues_ride_in_the_launch(T, split, mkn, epi, products):
    """plain: no worse than 4 x the default route's error on the same operands.  alpha, beta Cin (apart) through to_blas_gemm;
    P <- 0.75 P - 1.5 A B in place (aliasing); act(-1.5 W x + b) recorded in one scope: each fused into the product's launch"""
    from tensor_ops_amd import capi, hipt
    from tensor_ops_amd.hipt import DT
    m, k, n = mkn
    rng = np.random.default_rng(7400)
    a, b, c, bias = rng.uniform(-1, 1, (m, k)), rng.uniform(-1, 1, (k, n)), rng.uniform(-1, 1, (m, n)), rng.uniform(-1, 1, n)
    a, b, c, bias = (v.astype(F32) for v in (a, b, c, bias))
    prod = ld(a) @ ld(b)
    if epi == "plain":
        today = row_err(T.gmul(1, 1, 1, T.put(a), T.put(b)).numpy(), prod)
    split(2, products)
    bits = {"plain": (), "alpha": (), "beta": ("beta",), "alias": ("beta",), "logistic": ("bias", "act"), "tanh": ("bias", "act")}[epi]
    r = T.gemm_route(m, k, n, "f32", b_transposed=epi in ("logistic", "tanh"), epilogue=bits)
    assert r["families"] == [FAM] and r["epilogue_ok"] and not r["small_route"]
    if epi == "plain":
        da, db = T.put(a), T.put(b)
        st = T.stats()["launches"]
        got, want = T.gmul(1, 1, 1, da, db), prod
    elif epi in ("alpha", "beta"):
        h = capi.c_tensor()
        da, db, dc = T.put(a), T.put(b), T.put(c)
        st = T.stats()["launches"]
        capi.check(capi.lib().to_blas_gemm(0.5, da.h, db.h, 0.75, dc.h if epi == "beta" else None, C.byref(h)))
        got, want = DT(h), np.longdouble(0.5) * prod + (np.longdouble(0.75) * ld(c) if epi == "beta" else 0)
    elif epi == "alias":
        da, db, P = T.put(a), T.put(b), T.put(c)
        st = T.stats()["launches"]
        with T.memo():
            p2 = T.liftT(lambda v: 0.75 * v[0] - 1.5 * v[1], [P, T.gmul(1, 1, 1, da, db)], key="split-in-place")
            capi.check(capi.lib().to_copy_into(P.h, p2.h))
            del p2
        got, want = P, np.longdouble(0.75) * ld(c) - np.longdouble(1.5) * prod
    else:
        f = hipt.logistic_closure if epi == "logistic" else (lambda v: hipt.tanh(v[0]))
        dx, dw, dbias = T.put(a, batched=True), T.put(np.ascontiguousarray(b.T)), T.put(bias)
        st = T.stats()["launches"]
        with T.memo():
            got = T.force(T.liftT(f, [T.sumT([T.scaleT(-1.5, T.matVec(dw, dx)), dbias], (n,))], key="split-" + epi))
        z = np.longdouble(-1.5) * prod + ld(bias)
        want = 1 / (1 + np.exp(-z)) if epi == "logistic" else np.tanh(z)
    assert T.stats()["launches"] - st == 2
    err = row_err(got.numpy().reshape(m, n), want)
    assert err < 1e-5
    if epi == "plain":
        assert err <= 4 * today


@pytest.mark.parametrize("products", PRODUCTS)
def test_non_finite_operands(T, split, products):
    """+inf, -inf and a NaN in A: exactly the reference's elements are non-finite; FLT_MAX comes back finite and exact"""
    (m, k, n), rng = (37, 150, 70), np.random.default_rng(7500)
    a, b = rng.uniform(-1, 1, (m, k)).astype(F32), rng.uniform(-1, 1, (k, n)).astype(F32)
    a[3, 5], a[20, 149], a[36, 64] = np.inf, -np.inf, np.nan
    split(2, products)
    got = T.gmul(1, 1, 1, T.put(a), T.put(b)).numpy()
    with np.errstate(invalid="ignore"):
        want = ld(a) @ ld(b)
    assert np.array_equal(np.isfinite(got), np.isfinite(want)) and np.isfinite(got).sum() == (m - 3) * n
    a, b = rng.integers(0, 2, size=(m, k)).astype(F32), rng.integers(0, 2, size=(k, n)).astype(F32)
    a[11, :], a[11, 77] = 0, np.finfo(F32).max
    got = T.gmul(1, 1, 1, T.put(a), T.put(b)).numpy()
    assert np.all(np.isfinite(got)) and np.array_equal(got, (ld(a) @ ld(b)).astype(F32))


def test_the_switch_routes(T, split):
    from tensor_ops_amd import capi
    in_scope = ((4096, 4096, 4096), (37, 150, 70), (2, 3, 5))
    assert T.set_gemm_f32_split(0) == 0            # off is the default
    st = T.stats()["launches"]
    assert all(FAM not in T.gemm_route(m, k, n, "f32")["families"] for m, k, n in in_scope)
    split(2)
    assert all(T.gemm_route(m, k, n, "f32")["families"] == [FAM] for m, k, n in in_scope)
    # out of scope: fp64; a batch; the act' epilogue
    for dt, kw in (("f64", {}), ("f32", {"batch": 2}), ("f32", {"epilogue": ("dact",)})):
        assert FAM not in T.gemm_route(37, 150, 70, dt, **kw)["families"]
    # mode 1: the scanned rows that measured ahead (profiles/gemm_split_scan.txt: 4096^3 916 -> 705 us with six products, but 925
    # with nine; 2048^3 121 -> 185); 4000^3 was not scanned, nor 4096^3 transposed, with an epilogue or as a block of 4100 x 4096^2
    split(1)
    assert T.gemm_route(4096, 4096, 4096, "f32")["families"] == [FAM]
    for m, kw in ((2048, {}), (4000, {}), (4096, {"a_transposed": True}), (4096, {"epilogue": ("bias", "act")})):
        assert FAM not in T.gemm_route(m, m, m, "f32", **kw)["families"]
    assert FAM not in T.gemm_route(4100, 4096, 4096, "f32")["families"]
    split(1, 9)
    assert FAM not in T.gemm_route(4096, 4096, 4096, "f32")["families"]
    assert T.stats()["launches"] == st             # the query launches nothing
    # bad arguments: TO_ERR_ARG, nothing changed
    prev = C.c_int(-7)
    for mode, products in ((3, -1), (2, 3), (2, 7)):
        assert capi.lib().to_set_gemm_f32_split(mode, products, C.byref(prev)) == 1   # TO_ERR_ARG
    assert prev.value == -7 and T.set_gemm_f32_split(2, 9) == 1
    # a repeated call gives the same bits
    rng = np.random.default_rng(7600)
    da, db = T.put(rng.uniform(-1, 1, (257, 40)).astype(F32)), T.put(rng.uniform(-1, 1, (40, 129)).astype(F32))
    assert np.array_equal(T.gmul(1, 1, 1, da, db).numpy(), T.gmul(1, 1, 1, da, db).numpy())
