"""The few-right-hand-sides streaming kernel (`gemm_fewrhs_kernel`, csrc/gemm_fewrhs.hip; `to_set_gemm_few_rhs`): forced (mode
2) on all four operand layouts in both element types against a plain `np.longdouble` product -- bit-exact on small integers,
where every partial sum is exact whatever the order --, unsplit and with K split in three; every epilogue (alpha, bias +
activation, `beta Cin` with `Cin` apart from and aliasing `C`) at the project's bars; and the routing of the switch.  Every
test puts the previous mode back."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FAM = "fewrhs"
NP = {"f32": np.float32, "f64": np.float64}
BAR = {"f32": 1e-5, "f64": 1e-12}
ONE_CHUNK_K = {"f32": 128, "f64": 64}   # k of one LDS chunk at 32 columns: 16 KiB / (32 x element size) (the kernel's header)
LAYOUTS = [(0, 0), (0, 1), (1, 0), (1, 1)]


@pytest.fixture(scope="module")
def Ts():
    from tensor_ops_amd.hipt import HipT
    return {dt: HipT(0, dtype=NP[dt]) for dt in NP}


@pytest.fixture()
def few(Ts):
    """set(mode, splits) for the length of one test"""
    first = []

    def set_(mode, splits=-1):
        first.append(Ts["f32"].set_gemm_few_rhs(mode, splits))
    yield set_
    if first:
        Ts["f32"].set_gemm_few_rhs(first[0])


def ld(x):
    return x.astype(np.longdouble)


def operands(T, a, b, ta, tb):
    da = T.transp(T.put(np.ascontiguousarray(a.T))) if ta else T.put(a)
    db = T.transp(T.put(np.ascontiguousarray(b.T))) if tb else T.put(b)
    return da, db


def shapes(dt):
    """(m, k, n, splits): one row block under one MFMA k step; ragged rows, a K tail; one column block / two; 6 past an LDS
    chunk at 32 columns; whole 16-byte trips with full and ragged row blocks in both storage orders (132 x 80: every stride a
    multiple of 16 bytes); the narrow-M mirror; both extents narrow; K in three uneven parts, the last one short"""
    return [(16, 4, 2, -1), (18, 22, 10, -1), (37, 150, 16, -1), (37, 150, 17, -1), (70, ONE_CHUNK_K[dt] + 6, 32, -1),
            (132, 80, 5, -1), (10, 150, 70, -1), (32, 22, 37, -1), (2, 150, 2, -1), (37, 150, 17, 3), (10, 150, 70, 3)]


CASES = [(dt, s) for dt in NP for s in shapes(dt)]


@pytest.mark.parametrize("ta,tb", LAYOUTS)
@pytest.mark.parametrize("dt,mkns", CASES, ids=["%s-%dx%dx%d-s%d" % ((dt,) + s) for dt, s in CASES])
def test_forced_is_bit_exact_on_integers(Ts, few, dt, mkns, ta, tb):
    m, k, n, splits = mkns
    T = Ts[dt]
    rng = np.random.default_rng(7100 + 2 * ta + tb)
    a = rng.integers(-3, 4, size=(m, k)).astype(NP[dt])
    b = rng.integers(-3, 4, size=(k, n)).astype(NP[dt])
    few(2, splits)
    assert T.gemm_route(m, k, n, dt, a_transposed=bool(ta), b_transposed=bool(tb))["families"] == [FAM]
    da, db = operands(T, a, b, ta, tb)
    st = T.stats()["launches"]
    got = T.gmul(1, 1, 1, da, db)
    assert T.stats()["launches"] - st == (2 if splits > 0 else 1)
    assert np.array_equal(got.numpy(), (ld(a) @ ld(b)).astype(NP[dt]))


def row_err(got, want):
    """the bar of tests/test_gpu_f64.py, relative to the largest magnitude of each row"""
    return float(np.max(np.max(np.abs(got - want), axis=1) / np.max(np.abs(want), axis=1)))


def act_ref(act, z):
    return 1 / (1 + np.exp(-z)) if act == "logistic" else np.tanh(z)


EPI_SHAPES = [(37, 150, 10), (10, 150, 37)]


@pytest.mark.parametrize("splits", [-1, 3])
@pytest.mark.parametrize("epi", ["alpha", "beta", "alias", "logistic", "tanh"])
@pytest.mark.parametrize("mkn", EPI_SHAPES, ids=["%dx%dx%d" % s for s in EPI_SHAPES])
@pytest.mark.parametrize("dt", list(NP))
def test_epilogues_ride_in_the_launch(Ts, few, dt, mkn, epi, splits):
    """alpha through to_blas_gemm; beta Cin through to_blas_gemm (apart) and through P <- 0.75 P - 1.5 A B produced in place
    (aliasing); act(-1.5 W x + b) recorded in one scope over a batch: the planner fuses each into the product's own launch"""
    from tensor_ops_amd import capi, hipt
    from tensor_ops_amd.hipt import DT
    m, k, n = mkn
    T = Ts[dt]
    rng = np.random.default_rng(7200)
    a, b, c, bias = rng.uniform(-1, 1, (m, k)), rng.uniform(-1, 1, (k, n)), rng.uniform(-1, 1, (m, n)), rng.uniform(-1, 1, n)
    a, b, c, bias = (v.astype(NP[dt]) for v in (a, b, c, bias))
    few(2, splits)
    bits = {"alpha": (), "beta": ("beta",), "alias": ("beta",), "logistic": ("bias", "act"), "tanh": ("bias", "act")}[epi]
    r = T.gemm_route(m, k, n, dt, b_transposed=epi in ("logistic", "tanh"), epilogue=bits)
    assert r["families"] == [FAM] and r["epilogue_ok"] and not r["small_route"]
    prod = ld(a) @ ld(b)
    st = T.stats()["launches"]
    if epi in ("alpha", "beta"):
        h = capi.c_tensor()
        da, db, dc = T.put(a), T.put(b), T.put(c)
        st = T.stats()["launches"]
        capi.check(capi.lib().to_blas_gemm(0.5, da.h, db.h, 0.75, dc.h if epi == "beta" else None, C.byref(h)))
        got, want = DT(h), np.longdouble(0.5) * prod + (np.longdouble(0.75) * ld(c) if epi == "beta" else 0)
    elif epi == "alias":
        da, db, P = T.put(a), T.put(b), T.put(c)
        st = T.stats()["launches"]
        with T.memo():
            p2 = T.liftT(lambda v: 0.75 * v[0] - 1.5 * v[1], [P, T.gmul(1, 1, 1, da, db)], key="fewrhs-in-place")
            capi.check(capi.lib().to_copy_into(P.h, p2.h))
            del p2
        got, want = P, np.longdouble(0.75) * ld(c) - np.longdouble(1.5) * prod
    else:
        f = hipt.logistic_closure if epi == "logistic" else (lambda v: hipt.tanh(v[0]))
        dx, dw, dbias = T.put(a, batched=True), T.put(np.ascontiguousarray(b.T)), T.put(bias)
        st = T.stats()["launches"]
        with T.memo():
            got = T.force(T.liftT(f, [T.sumT([T.scaleT(-1.5, T.matVec(dw, dx)), dbias], (n,))], key="fewrhs-" + epi))
        want = act_ref(epi, np.longdouble(-1.5) * prod + ld(bias))
    assert T.stats()["launches"] - st == (2 if splits > 0 else 1)
    assert row_err(got.numpy().reshape(m, n), want.astype(NP[dt])) < BAR[dt]


def test_the_switch_routes(Ts, few):
    from tensor_ops_amd import capi
    T = Ts["f32"]
    assert T.set_gemm_few_rhs(0) == 0            # off is the default
    st = T.stats()["launches"]
    for dt in NP:
        for m, k, n in ((60000, 100, 10), (37, 150, 17)):
            assert FAM not in T.gemm_route(m, k, n, dt)["families"]
    few(2)
    for dt in NP:
        for m, k, n in ((60000, 100, 10), (37, 150, 17)):
            assert T.gemm_route(m, k, n, dt)["families"] == [FAM]
        # out of range: both extents above 32; one right-hand side; a batch; the act' epilogue
        assert FAM not in T.gemm_route(33, 150, 33, dt)["families"]
        assert FAM not in T.gemm_route(60000, 100, 1, dt)["families"]
        assert FAM not in T.gemm_route(37, 150, 17, dt, batch=2)["families"]
        assert FAM not in T.gemm_route(37, 150, 17, dt, epilogue=("dact",))["families"]
    # mode 1: the scanned rows that measured ahead (profiles/gemm_fewrhs_scan.txt: 60000 x 100 x 10 22.5 -> 10.7 us in fp32, 60000 x
    # 300 x 32 52.5 -> 32.3 in fp64 but 23.0 -> 27.8 in fp32); 50000 x 100 x 10 was not scanned
    few(1)
    assert T.gemm_route(60000, 100, 10, "f32")["families"] == [FAM] and T.gemm_route(60000, 300, 32, "f64")["families"] == [FAM]
    assert FAM not in T.gemm_route(60000, 300, 32, "f32")["families"] + T.gemm_route(50000, 100, 10, "f32")["families"]
    assert T.stats()["launches"] == st           # the query launches nothing
    # bad arguments: TO_ERR_ARG, nothing changed
    prev = C.c_int(-7)
    for mode, splits in ((3, -1), (2, 0), (2, 257), (2, -2)):
        assert capi.lib().to_set_gemm_few_rhs(mode, splits, C.byref(prev)) == 1   # TO_ERR_ARG
    assert prev.value == -7 and T.set_gemm_few_rhs(2) == 1
