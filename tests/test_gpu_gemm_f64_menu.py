"""The fp64 tile menu (`gemm_kw64_menu_kernel`, csrc/gemm_kwave_f64.hip; `to_set_gemm_f64_menu`): every menu tile forced
(mode 2) on all four operand layouts against a plain `np.longdouble` product -- bit-exact on small integers, where every
partial sum is exact in fp64 whatever the order --, every epilogue (alpha, bias + activation, `act'`, `beta Cin` with `Cin`
apart from and aliasing `C`) at the project's fp64 bar, and the routing of the switch.  Every test puts the previous mode back."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TILES = [(48, 48), (48, 64), (64, 48), (32, 64), (64, 32)]   # menu index -> (BM, BN)
MENU = "kw16_64"


@pytest.fixture(scope="module")
def T():
    from tensor_ops_amd.hipt import HipT
    return HipT(0, dtype=np.float64)


@pytest.fixture()
def menu(T):
    """set(mode, tile) for the length of one test"""
    first = []

    def set_(mode, tile=-1):
        first.append(T.set_gemm_f64_menu(mode, tile))
    yield set_
    if first:
        T.set_gemm_f64_menu(first[0])


def ref(a, b):
    return (a.astype(np.longdouble) @ b.astype(np.longdouble)).astype(np.float64)


def operands(T, a, b, ta, tb):
    da = T.transp(T.put(np.ascontiguousarray(a.T))) if ta else T.put(a)
    db = T.transp(T.put(np.ascontiguousarray(b.T))) if tb else T.put(b)
    return da, db


def shapes(bm, bn):
    """(m, k, n): one exact tile under one k-tile (three idle waves); a ragged second tile each way, uneven runs; an odd N (scalar
    stores; an n-contiguous B with an odd N is outside the kernel's range and keeps its route); 5 x 2 tiles less six rows
    (a partial last band, ntiles & 7 != 0 over more than 8 tiles) under nine k-tiles = 16 (4 NI + 1): the ring wraps in
    every wave; a K tail of 6."""
    return [(bm, 16, bn), (bm + 2, 48, bn + 2), (bm + 2, 144, bn + 3), (5 * bm - 6, 144, 2 * bn), (bm + 2, 150, bn + 2)]


CASES = [(t, s) for t, (bm, bn) in enumerate(TILES) for s in shapes(bm, bn)]


@pytest.mark.parametrize("ta,tb", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("tile,mkn", CASES, ids=["%dx%d-%dx%dx%d" % (TILES[t] + s) for t, s in CASES])
def test_forced_tile_is_bit_exact_on_integers(T, menu, tile, mkn, ta, tb):
    m, k, n = mkn
    rng = np.random.default_rng(6400 + 8 * tile + 2 * ta + tb)
    a = rng.integers(-3, 4, size=(m, k)).astype(np.float64)
    b = rng.integers(-3, 4, size=(k, n)).astype(np.float64)
    menu(2, tile)
    fam = T.gemm_route(m, k, n, "f64", a_transposed=bool(ta), b_transposed=bool(tb))["families"]
    in_range = (m % 2 == 0 or not ta) and (n % 2 == 0 or tb)   # a contiguous pair is in or out of the matrix as a whole
    assert (fam == [MENU]) == in_range, fam
    da, db = operands(T, a, b, ta, tb)
    assert np.array_equal(T.gmul(1, 1, 1, da, db).numpy(), ref(a, b))


def row_err(got, want):
    """the fp64 bar of tests/test_gpu_f64.py (1e-12), relative to the largest magnitude of each row"""
    return float(np.max(np.max(np.abs(got - want), axis=1) / np.max(np.abs(want), axis=1)))


@pytest.mark.parametrize("ta,tb", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_alpha_and_beta_cin_on_48x48(T, menu, ta, tb):
    """to_blas_gemm: alpha = -1.5, beta = 0.75 with an addend, 100 x 144 x 52 (3 x 2 tiles, ragged both ways)"""
    from tensor_ops_amd import capi
    from tensor_ops_amd.hipt import DT
    rng = np.random.default_rng(6500 + 2 * ta + tb)
    a, b, c = rng.uniform(-1, 1, (100, 144)), rng.uniform(-1, 1, (144, 52)), rng.uniform(-1, 1, (100, 52))
    menu(2, 0)
    da, db = operands(T, a, b, ta, tb)
    h = capi.c_tensor()
    capi.check(capi.lib().to_blas_gemm(-1.5, da.h, db.h, 0.75, T.put(c).h, C.byref(h)))
    want = (np.longdouble(-1.5) * (a.astype(np.longdouble) @ b.astype(np.longdouble)) + np.longdouble(0.75) * c).astype(np.float64)
    assert row_err(DT(h).numpy(), want) < 1e-12


@pytest.mark.parametrize("ta,tb", [(0, 0), (1, 1)])
def test_beta_cin_aliasing_c_on_48x48(T, menu, ta, tb):
    """P <- 0.75 P - 1.5 A B recorded in one scope and copied into P's own storage: ONE launch that reads Cin = C = P element
    for element (the planner produces it in place), 100 x 144 x 52"""
    from tensor_ops_amd import capi
    rng = np.random.default_rng(6550 + ta)
    a, b, c = rng.uniform(-1, 1, (100, 144)), rng.uniform(-1, 1, (144, 52)), rng.uniform(-1, 1, (100, 52))
    menu(2, 0)
    r = T.gemm_route(100, 144, 52, "f64", a_transposed=bool(ta), b_transposed=bool(tb), epilogue=("beta",))
    assert r["families"] == [MENU] and r["epilogue_ok"] and not r["small_route"]
    da, db = operands(T, a, b, ta, tb)
    P = T.put(c)
    st = T.stats()["launches"]
    with T.memo():
        p2 = T.liftT(lambda v: 0.75 * v[0] - 1.5 * v[1], [P, T.gmul(1, 1, 1, da, db)], key="menu-in-place")
        capi.check(capi.lib().to_copy_into(P.h, p2.h))
        del p2
    assert T.stats()["launches"] - st == 1
    want = (np.longdouble(0.75) * c - np.longdouble(1.5) * (a.astype(np.longdouble) @ b.astype(np.longdouble))).astype(np.float64)
    assert row_err(P.numpy(), want) < 1e-12


def act_ref(act, z):
    return 1 / (1 + np.exp(-z)) if act == "logistic" else np.tanh(z)


@pytest.mark.parametrize("act", ["logistic", "tanh"])
def test_alpha_bias_and_activation_ride_in_the_launch_on_48x48(T, menu, act):
    """act(-1.5 W x + b) recorded in one scope over a 100-row batch, 144 -> 52: ONE launch, the menu kernel's (the plan says so)"""
    from tensor_ops_amd import hipt
    rng = np.random.default_rng(6600)
    x, w, bias = rng.uniform(-1, 1, (100, 144)), rng.uniform(-1, 1, (52, 144)), rng.uniform(-1, 1, 52)
    menu(2, 0)
    r = T.gemm_route(100, 144, 52, "f64", b_transposed=True, epilogue=("bias", "act"))
    assert r["families"] == [MENU] and r["epilogue_ok"] and not r["small_route"]
    f = hipt.logistic_closure if act == "logistic" else (lambda v: hipt.tanh(v[0]))
    dx, dw, db = T.put(x, batched=True), T.put(w), T.put(bias)
    st = T.stats()["launches"]
    with T.memo():
        got = T.force(T.liftT(f, [T.sumT([T.scaleT(-1.5, T.matVec(dw, dx)), db], (52,))], key="menu-" + act))
    assert T.stats()["launches"] - st == 1
    z = np.longdouble(-1.5) * (x.astype(np.longdouble) @ w.T.astype(np.longdouble)) + bias
    assert row_err(got.numpy().reshape(100, 52), act_ref(act, z).astype(np.float64)) < 1e-12


@pytest.mark.parametrize("act", ["logistic", "tanh"])
def test_dact_rides_in_the_launch_on_48x48(T, menu, act):
    """h = act(W1 x + b1) and dz1 = (W2^T dz2) * act'(W1 x + b1), 100 rows, 144 -> 52, recorded in one scope: the planner hands h
    to the backward product as its `dact` operand -- TWO launches, the forward's and the backward's, both the menu kernel's"""
    from tensor_ops_amd import hipt
    rng = np.random.default_rng(6700)
    x, w1, b1 = rng.uniform(-1, 1, (100, 16)), rng.uniform(-1, 1, (52, 16)), rng.uniform(-1, 1, 52)
    dz2, w2 = rng.uniform(-1, 1, (100, 144)), rng.uniform(-1, 1, (144, 52))
    menu(2, 0)
    r = T.gemm_route(100, 144, 52, "f64", epilogue=("dact",))
    assert r["families"] == [MENU] and r["epilogue_ok"] and not r["small_route"]
    if act == "logistic":
        f = hipt.logistic_closure
        df = lambda v: v[0] * (f(v[1:]) * (1.0 - f(v[1:])))   # noqa: E731
    else:
        f = lambda v: hipt.tanh(v[0])   # noqa: E731
        df = lambda v: v[0] * (1.0 - hipt.tanh(v[1]) * hipt.tanh(v[1]))   # noqa: E731
    dx, dw1, db1, ddz2, dw2 = T.put(x, batched=True), T.put(w1), T.put(b1), T.put(dz2, batched=True), T.put(w2)
    st = T.stats()["launches"]
    with T.memo():
        z = T.sumT([T.matVec(dw1, dx), db1], (52,))
        h = T.liftT(f, [z], key="menu-fwd-" + act)
        dz1 = T.liftT(df, [T.matVec(T.transp(dw2), ddz2), z], key="menu-d" + act)
        del z
        T.force_many([h, dz1])
    assert T.stats()["launches"] - st == 2
    hh = act_ref(act, x.astype(np.longdouble) @ w1.T.astype(np.longdouble) + b1)
    d = dz2.astype(np.longdouble) @ w2.astype(np.longdouble)
    want = d * (hh * (1 - hh) if act == "logistic" else 1 - hh * hh)
    assert row_err(h.numpy().reshape(100, 52), hh.astype(np.float64)) < 1e-12
    assert row_err(dz1.numpy().reshape(100, 52), want.astype(np.float64)) < 1e-12


ROUTED = [(768, 768, 768), (1280, 1280, 1280), (1024, 1024, 512)]   # (m, k, n); the parent sends all three to kw64


def test_the_switch_routes(T, menu):
    from tensor_ops_amd import capi
    assert T.set_gemm_f64_menu(0) == 0            # off is the default
    for m, k, n in ROUTED:
        assert T.gemm_route(m, k, n, "f64")["families"] == ["kw64"]
    menu(2)
    for m, k, n in ROUTED:
        assert T.gemm_route(m, k, n, "f64")["families"] == [MENU]
    assert T.gemm_route(768, 768, 768, "f32")["families"] == ["kw16"]        # fp32 is not the menu's business
    assert T.gemm_route(768, 768, 768, "f64", epilogue=("rowsum",))["families"] != [MENU]
    # mode 1: exactly what the fitted rule claims -- profiles/gemm_f64_menu_scan.txt: 768^3 26.9 -> 17.2 us on 48x48, 1024 x 1024 x
    # 512 33.7 -> 19.0 on 64x32 (and 1280^3 80.1 -> 72.6); 1024^3 measured behind (34.4 -> 36.4), 800^3 was not scanned
    menu(1)
    for m, k, n in ROUTED:
        assert T.gemm_route(m, k, n, "f64")["families"] == [MENU]
    assert T.gemm_route(1024, 1024, 1024, "f64")["families"] == ["kw64"]
    assert T.gemm_route(800, 800, 800, "f64")["families"] == ["kw64"]
    # bad arguments: TO_ERR_ARG, nothing changed
    prev = C.c_int(-7)
    for mode, tile in ((3, -1), (-1, -1), (2, 5), (2, -2)):
        assert capi.lib().to_set_gemm_f64_menu(mode, tile, C.byref(prev)) == 1   # TO_ERR_ARG
    assert prev.value == -7 and T.set_gemm_f64_menu(1) == 1
