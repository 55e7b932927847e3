"""The row programs of csrc/rowprog.cpp -- a row-local subgraph of the recorded stream printed as HIP source, compiled by hiprtc
and run as one kernel, a wave per row -- op by op, at every width, in both element types.  Programs, formation rule and
references: tests/rowprog_cases.py (checked on the CPU by tests/test_rowprog_cases.py).

Every case is recorded inside `T.memo()` behind one contraction z = W x, its outputs demanded together into memory that held
NaN, and held to three things: every demanded value equals the reference (bit for bit on exact data); the launch count is the
contraction's own plus what the restated formation rule says (1 for a program, one per op without: a silent fall back to
op-by-op fails here); `to_lazy_stats`' elided counter rises by the members a program keeps to itself, and only then.

 a. one program per RowOp at N = 65, B = 5, each twice in a row (the second from the plan cache), one again at another B
 b. widths 1 .. 1024 and 1025 (no program), batches 1 .. 130 and the unbatched root: an exact program with a row sum, a dot
    product against one-hot probes and a vector output, and the 19-op softmax >>> scale >>> squaredError head
 c. dead lanes: exp 0, 1 / 0 and log 0 in the lanes past N beside a row sum
 d. the kinds of external operand, a peer, and the limits of 4 operands and 4 outputs
 e. NaN, +inf, -inf in z; an infinite R_SCALE factor and R_CONST
 f. the composite head on random data, per element against float64 / long double
 g. one fp32 head at N = 784 captured in a HIP graph and replayed
 h. everything of a, b, e and f again with TOPS_ROWPROG=0 (read once per process): ONE child process (this file as a script)
    under a time limit of its own; the *_off tests read its report

Measured on an MI355X, largest |got - ref| / max(1, |ref|) per element of section f (random rows, N = 65, 784, 1024):
fp32 6.84e-08 with programs, 5.16e-07 op by op (bound 1e-5); fp64 9.16e-17 with programs, 1.86e-15 op by op (bound 1e-12).
Over the width table the composite stays below 1.3e-07 (fp32) and 2e-16 (fp64) with a program and reaches 1.99e-06 / 2.46e-15
at N = 1025, where there is none.  The file takes 12 s, the child included (80 hiprtc builds: 48 fp32 programs, 31 fp64, one
captured step; the fp64 width list is short -- 65, 1000, 1024, 1025 -- to stay at that number of builds, not for time).
With csrc/rowprog.cpp as it is, five hand-made mutations each fail here: the R_SUM_ROWS guard dropped (37 tests), the root
loaded with EPL - 1 trips (25), the two R_DACT forms swapped (2), a shared external read per row (10), the admission limit
raised to 2048 (4).  No test exposed a defect in the generator, the formation rule or run_rowprog.

The suspects read while writing this file, none of them a defect: (1) a closure of arity 0 -- the recorder cannot produce
one (`to_lift` refuses n = 0), no case; (2) the retry without peers -- an op that reads a peer is not a member then, so a
program of the retry cannot read a peer it dropped: case `peer-5` holds the count and the values; (3) R_LIFT as a scalar
node -- `to_lift` demands operands of one shape, so a scalar lift has scalar inputs only: case `lift-scalar`; (4) fp64 at
EPL = 16 with the composite's 19 live vectors -- right values at N = 1000 and 1024 (sections b and f)."""
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import rowprog_cases as RP  # noqa: E402

try:
    import pytest
    pytestmark = pytest.mark.gpu
except ImportError:          # (the child needs none of it)
    pytest = None

NAN = np.nan
_T = {}
_T0 = time.time()


def backend(dt):
    from tensor_ops_amd.hipt import HipT
    dt = np.dtype(dt).type
    if dt not in _T:
        _T[dt] = HipT(0, dt)
    return _T[dt]


def lazy_stats():
    from tensor_ops_amd import capi
    a = [C.c_int64() for _ in range(4)]
    capi.check(capi.lib().to_lazy_stats(*[C.byref(v) for v in a]))
    return dict(zip(("recorded", "fused_launches", "elided", "flushes"), [v.value for v in a]))


def plan_cache_stats():
    from tensor_ops_amd import capi
    a = [C.c_int64() for _ in range(3)]
    capi.check(capi.lib().to_plan_cache_stats(*[C.byref(v) for v in a]))
    return dict(zip(("hits", "misses", "entries"), [v.value for v in a]))


def nan_pool(T, *counts):
    """upload and release NaN-filled tensors of the sizes about to be asked for: the pool memory handed out next is NaN, so an
    element no lane writes shows"""
    held = [T.put(np.full(int(n), NAN, T.dtype.type)) for n in counts for _ in range(2) if n > 0]
    T.sync()
    del held


class SymMath:
    """the closures' math on the symbolic values of tensor_ops_amd.hipt"""
    @staticmethod
    def _h():
        from tensor_ops_amd import hipt
        return hipt

    max = staticmethod(lambda a, b: SymMath._h().maximum(a, b))
    min = staticmethod(lambda a, b: SymMath._h().minimum(a, b))
    abs = staticmethod(abs)
    exp = staticmethod(lambda a: SymMath._h().exp(a))
    log = staticmethod(lambda a: SymMath._h().log(a))
    tanh = staticmethod(lambda a: SymMath._h().tanh(a))
    recip = staticmethod(lambda a: SymMath._h().recip(a))


class Dev:
    """the programs of rowprog_cases on device handles: every method records one class-method call"""

    def __init__(self, T):
        self.T = T

    def liftT(self, f, xs):
        return self.T.liftT(lambda v: f.fn(SymMath, v), xs, key=("rowprog", f.name))

    def gmul(self, lm, lo, ln, x, y):
        return self.T.gmul(lm, lo, ln, x, y)

    def sumT(self, xs, shape):
        return self.T.sumT(xs, shape)

    def scaleT(self, alpha, x):
        return self.T.scaleT(alpha, x)

    def sumRows(self, x):
        return self.T.sumRows(x)

    def mapRows_const(self, len_n, row, like):
        return self.T.mapRows_const(len_n, row, like)

    def konst(self, shape, c):
        return self.T.konst(shape, c)


_CONTRACTION = {}


def contraction_launches(T, dW, dx, key):
    """what z = W x costs on its own, measured once per shape outside a scope: the counts below are held BEHIND it"""
    if key not in _CONTRACTION:
        before = T.stats()["launches"]
        T.matVec(dW, dx)
        _CONTRACTION[key] = T.stats()["launches"] - before
    return _CONTRACTION[key]


def upload(T, case, B, N, x=None):
    W, x0 = RP.root_data(case, B, N)
    x = x0 if x is None else (x if B > 0 else x[0])
    dW, dx = T.put(W), T.put(x, batched=B > 0)
    v = {"n": N}
    for name, (kind, a) in RP.operands(case, B, N).items():
        per_row = kind in ("vec_row", "sc_row", "probe")
        v[name] = T.put(a if (B > 0 or not per_row) else a[0], batched=per_row and B > 0)
    roots = [(dW, dx)]
    if case.get("peer"):
        Wp, s = RP.peer_data(B, N)
        roots.append((T.put(Wp), T.put(s if B > 0 else s[0], batched=B > 0)))
    return roots, v


def run_case(T, case, B, N, fails, ctx, x=None, rowprog_on=True, exact=True):
    """record, demand, count and compare one case; returns the downloaded outputs"""
    dt = T.dtype.type
    ctx = "%s %s N=%d B=%d" % (ctx, case["id"], N, B)
    roots, v = upload(T, case, B, N, x)
    behind = sum(contraction_launches(T, dW, dx, (dt, N, B, i)) for i, (dW, dx) in enumerate(roots))
    want, _ = RP.reference(case, B, N, x=x)
    rows = max(B, 1)
    nan_pool(T, rows * N, rows * N, rows)
    s0, l0 = lazy_stats(), T.stats()["launches"]
    with T.memo():
        v["z"] = T.matVec(*roots[0])
        if case.get("peer"):
            v["p"] = T.matVec(*roots[1])
        outs = case["build"](Dev(T), v)
        T.force_many(outs)
        launched = T.stats()["launches"] - l0
        got = [o.numpy() for o in outs]
        del v, outs
    s1 = lazy_stats()
    expected = behind + RP.launches(case, N, rowprog_on)
    if launched != expected:
        fails.append("%s: %d launches, the formation rule says %d" % (ctx, launched, expected))
    if s1["elided"] - s0["elided"] != RP.elided(case, N, rowprog_on):
        fails.append("%s: elided rose by %d, expected %d" % (ctx, s1["elided"] - s0["elided"], RP.elided(case, N, rowprog_on)))
    for k, (g, w) in enumerate(zip(got, want)):
        w = np.asarray(w, dtype=np.float64)
        same = np.array_equal(g, w.astype(dt)) if exact else RP.same_with_nan(g, w.astype(dt))
        if g.shape != w.shape or not same:
            bad = np.flatnonzero(~((g.ravel() == w.ravel()) | (np.isnan(g.ravel()) & np.isnan(w.ravel()))))[:5] if g.shape == w.shape else []
            fails.append("%s: output %d differs at %s" % (ctx, k, [(int(i), float(w.ravel()[i]), float(g.ravel()[i])) for i in bad] or (g.shape, w.shape)))
    return got


# ---- the composite head ---------------------------------------------------------------------------------------------------------
def composite_data(B, N, rng=None):
    """(W, x, y): the exact integers and dyadic targets of the width table, or random rows (section f)"""
    rows = max(B, 1)
    if rng is None:
        W, x, y = RP.w_ints(N), RP.x_ints(rows) / 4.0, RP.dyadic(rows * N).reshape(rows, N)
    else:
        W, x, y = rng.uniform(-1, 1, (N, RP.K)), rng.uniform(-1, 1, (rows, RP.K)), rng.uniform(0, 1, (rows, N))
    return (W, x, y) if B > 0 else (W, x[0], y[0])


def run_composite(T, B, N, fails, ctx, rng=None, rowprog_on=True):
    """softmax >>> scale 0.5 >>> squaredError behind z = W x, value and cotangent, built by the host mirror the way
    test_unrecognised_networks_still_run_correctly builds it; returns the largest error per element"""
    from tensor_ops_amd import tops as H
    H.hlib()
    dt = T.dtype.type
    ctx = "%s composite N=%d B=%d" % (ctx, N, B)
    W, x, y = composite_data(B, N, rng)
    dW, dx, dy = T.put(W), T.put(x, batched=B > 0), T.put(y, batched=B > 0)
    behind = contraction_launches(T, dW, dx, (dt, N, B, 0))
    work = np.float64 if dt == np.float32 else np.longdouble
    # the reference starts from the operands as the device holds them
    Wd, xd, yd = (np.asarray(a, dtype=dt).astype(work) for a in (W, x, y))
    want = RP.composite_reference(xd @ Wd.T, yd, work)
    head = H.firstOp(H.softmax() >> H.scale(0.5), 1) >> H.squaredError()
    rows = max(B, 1)
    nan_pool(T, rows * N, rows * N, rows)
    H.set_elem_dtype(dt)
    try:
        s0, l0 = lazy_stats(), T.stats()["launches"]
        with T.memo():
            z = T.matVec(dW, dx)
            loss = head.run([z, dy])[0]
            dz = head.gradTOp([z, dy], want=[1, 0])[0]
            T.force_many([loss, dz])
            launched = T.stats()["launches"] - l0
            got = [loss.numpy(), dz.numpy()]
            del z, loss, dz
        s1 = lazy_stats()
    finally:
        H.set_elem_dtype(np.float32)
    expected = behind + RP.composite_launches(N, rowprog_on)
    if launched != expected:
        fails.append("%s: %d launches, the formation rule says %d" % (ctx, launched, expected))
    if s1["elided"] - s0["elided"] != RP.composite_elided(N, rowprog_on):
        fails.append("%s: elided rose by %d, expected %d" % (ctx, s1["elided"] - s0["elided"], RP.composite_elided(N, rowprog_on)))
    worst = 0.0
    for name, g, w in zip(("loss", "dz"), got, want):
        ok, err = RP.within(g, w, RP.TOL[dt])
        worst = max(worst, err)
        if not ok:
            fails.append("%s: %s off by %.3g per element (bound %g)" % (ctx, name, err, RP.TOL[dt]))
    return worst


# ---- the tables, shared by the parent (programs on) and the child (programs off) ---------------------------------------------------
def run_ops(dt, on, fails):
    T = backend(dt)
    for case in RP.OP_CASES:
        c0 = plan_cache_stats()
        first = run_case(T, case, RP.OP_B, RP.OP_N, fails, "ops", rowprog_on=on)
        again = run_case(T, case, RP.OP_B, RP.OP_N, fails, "ops again", rowprog_on=on)      # g: the second run, from the plan cache
        c1 = plan_cache_stats()
        if c1["hits"] - c0["hits"] < 1:
            fails.append("%s: the second run was planned afresh (%s -> %s)" % (case["id"], c0, c1))
        if any(not np.array_equal(a, b) for a, b in zip(first, again)):
            fails.append("%s: the second run gives other values" % case["id"])
    run_case(T, RP.OP_CASES[0], 3, RP.OP_N, fails, "ops at another B", rowprog_on=on)


def run_width(dt, N, B, on, fails):
    T = backend(dt)
    run_case(T, RP.WIDTH_CASE, B, N, fails, "widths", rowprog_on=on)
    return run_composite(T, B, N, fails, "widths", rowprog_on=on)


def run_nonfinite(dt, on, fails):
    T = backend(dt)
    x, clean = RP.poisoned_x(RP.OP_B)
    got = run_case(T, RP.NONFINITE_CASE, RP.OP_B, RP.OP_N, fails, "non-finite", x=x, rowprog_on=on, exact=False)
    plain = run_case(T, RP.NONFINITE_CASE, RP.OP_B, RP.OP_N, fails, "finite", rowprog_on=on)
    for g, p in zip(got, plain):
        if not np.array_equal(g[list(clean)], p[list(clean)]):
            fails.append("non-finite: a row without poison changed")
    run_case(T, RP.INF_CASE, RP.OP_B, RP.OP_N, fails, "literals", rowprog_on=on, exact=False)


def run_inexact(dt, on, fails):
    T = backend(dt)
    rng = np.random.default_rng(0x7e5000b1)
    return max(run_composite(T, RP.OP_B, N, fails, "random", rng=rng, rowprog_on=on) for N in RP.INEXACT_WIDTHS)


# ---- the child: every table with TOPS_ROWPROG=0 ------------------------------------------------------------------------------------
def off_child():
    report = {}

    def section(key, fn):
        fails = []
        try:
            worst = fn(fails)
        except Exception as err:  # noqa: BLE001
            worst = None
            fails.append("exception: %r" % (err,))
        report[key] = {"fails": fails[:12], "worst": worst}

    for dt, name in zip(RP.DTYPES, RP.DT_IDS):
        section("ops-" + name, lambda f: run_ops(dt, False, f))
        for N, B in RP.width_shapes(dt):
            section("width-%s-%d-%d" % (name, N, B), lambda f: run_width(dt, N, B, False, f))
        section("nonfinite-" + name, lambda f: run_nonfinite(dt, False, f))
        section("inexact-" + name, lambda f: run_inexact(dt, False, f))
    print("OFFREPORT " + json.dumps(report))


if __name__ == "__main__":
    off_child()
    sys.exit(0)


@pytest.fixture(scope="module")
def off_report():
    env = dict(os.environ, TOPS_ROWPROG="0", PYTHONPATH=ROOT)
    out = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, cwd=ROOT)
    if out.returncode < 0 or out.returncode in (124, 134, 137, 139):      # a fault or a hang: nothing more on this device
        pytest.exit("the child without row programs ended with %d: %s" % (out.returncode, (out.stdout + out.stderr)[-1500:]), returncode=3)
    line = [l for l in out.stdout.splitlines() if l.startswith("OFFREPORT ")]
    assert out.returncode == 0 and line, out.stdout[-2000:] + out.stderr[-2000:]
    return json.loads(line[-1][len("OFFREPORT "):])


DT = pytest.mark.parametrize("dt", RP.DTYPES, ids=RP.DT_IDS)
_WORST = {}


def _shape_params():
    return [pytest.param(dt, N, B, id="%s-N%d-B%d" % (n, N, B)) for dt, n in zip(RP.DTYPES, RP.DT_IDS) for N, B in RP.width_shapes(dt)]


def _name(dt):
    return RP.DT_IDS[RP.DTYPES.index(dt)]


# ---- a. one program per RowOp (g: twice in a row, once more at another B) -----------------------------------------------------------
@DT
def test_every_row_op_in_a_program_of_its_own(dt):
    fails = []
    run_ops(dt, True, fails)
    assert not fails, fails


@DT
def test_every_row_op_off(off_report, dt):
    r = off_report["ops-" + _name(dt)]
    assert r["fails"] == [], r["fails"]


# ---- b. widths, batches, the unbatched root ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,N,B", _shape_params())
def test_widths_and_batches(dt, N, B):
    fails = []
    worst = run_width(dt, N, B, True, fails)
    print("composite %s N=%d B=%d: largest error per element %.3g" % (_name(dt), N, B, worst))
    assert not fails, fails


@pytest.mark.parametrize("dt,N,B", _shape_params())
def test_widths_and_batches_off(off_report, dt, N, B):
    r = off_report["width-%s-%d-%d" % (_name(dt), N, B)]
    assert r["fails"] == [], r["fails"]
    # strictly more launches than with programs on, wherever one forms
    assert RP.launches(RP.WIDTH_CASE, N, False) > RP.launches(RP.WIDTH_CASE, N) or N > RP.MAX_N


# ---- c. dead lanes ------------------------------------------------------------------------------------------------------------------
@DT
@pytest.mark.parametrize("N", RP.DEAD_WIDTHS)
@pytest.mark.parametrize("case", RP.DEAD_CASES, ids=[c["id"] for c in RP.DEAD_CASES])
def test_dead_lanes_stay_out_of_a_row_sum(case, N, dt):
    """s = N exactly (a leaked lane adds 1, inf or -inf) and p = 1 / N, one correctly rounded division, bit for bit"""
    T = backend(dt)
    fails = []
    s, p = run_case(T, case, RP.OP_B, N, fails, "dead lanes")
    assert not fails, fails
    assert np.array_equal(s, np.full(RP.OP_B, N, dtype=dt))
    assert np.array_equal(p, np.full((RP.OP_B, N), dt(1) / dt(N), dtype=dt))


# ---- d. external operands and the limits ------------------------------------------------------------------------------------------------
@DT
@pytest.mark.parametrize("case", RP.EXT_CASES, ids=[c["id"] for c in RP.EXT_CASES])
def test_external_operands_and_limits(case, dt):
    T = backend(dt)
    fails = []
    run_case(T, case, RP.OP_B, RP.OP_N, fails, "externals")
    assert not fails, fails


# ---- e. non-finite values ---------------------------------------------------------------------------------------------------------------
@DT
def test_non_finite_values_inside_a_program(dt):
    fails = []
    run_nonfinite(dt, True, fails)
    assert not fails, fails


@DT
def test_non_finite_values_off(off_report, dt):
    r = off_report["nonfinite-" + _name(dt)]
    assert r["fails"] == [], r["fails"]


# ---- f. inexact closures ------------------------------------------------------------------------------------------------------------------
@DT
def test_composite_head_on_random_rows(dt):
    fails = []
    worst = run_inexact(dt, True, fails)
    print("random rows %s: largest error per element %.3g (bound %g)" % (_name(dt), worst, RP.TOL[dt]))
    assert not fails, fails


@DT
def test_composite_head_on_random_rows_off(off_report, dt):
    r = off_report["inexact-" + _name(dt)]
    print("random rows %s, programs off: largest error per element %s (bound %g)" % (_name(dt), r["worst"], RP.TOL[dt]))
    assert r["fails"] == [], r["fails"]


# ---- g. a program inside a captured step ----------------------------------------------------------------------------------------------------
def flat_grads(tr):
    from tensor_ops_amd import capi
    _, g_ptr, n = tr.flat()
    flat = np.empty(n, dtype=np.float32)
    h = capi.c_tensor()
    d = (C.c_int64 * 1)(n)
    capi.check(capi.lib().to_wrap(C.c_void_p(g_ptr), 0, 1, d, 0, C.byref(h)))
    capi.check(capi.lib().to_download(h, flat.ctypes.data_as(C.c_void_p), flat.nbytes))
    capi.lib().to_release(h)
    return flat


def test_a_program_replayed_from_a_captured_step():
    """tanh 30 -> 17 -> 784, softmax, scale, squaredError: the gradient issued directly and replayed three times from a HIP
    graph, bit for bit the same"""
    from tensor_ops_amd import tops as H
    H.hlib()
    T = backend(np.float32)
    rng = np.random.default_rng(0x7e5000b2)
    B, i, h, o = 5, 30, 17, 784
    ws = [(0.5 * rng.standard_normal((h, i)), 0.5 * rng.standard_normal(h)), (0.5 * rng.standard_normal((o, h)), 0.5 * rng.standard_normal(o))]
    X, Y = rng.uniform(0, 1, (B, i)), rng.uniform(0, 1, (B, o))
    grads = []
    for graph in (False, True):
        net = H.net_then(H.genNet([(T.put(w), T.put(b)) for w, b in ws], "actMapTanh", "actSoftmax"), H.scale(0.5))
        s0 = lazy_stats()
        tr = H.Trainer(net, "squaredError", 0.01, T.put(X, batched=True), T.put(Y, batched=True), use_graph=graph)
        assert lazy_stats()["elided"] > s0["elided"] and tr.launches_per_step <= 6, tr.launches_per_step
        assert tr.graph == graph
        for _ in range(3 if graph else 1):
            tr.grad()
            grads.append(flat_grads(tr))
    assert np.isfinite(grads[0]).all() and np.abs(grads[0]).max() > 0
    for g in grads[1:]:
        assert np.array_equal(g, grads[0])


def test_wall_time_of_this_file():
    print("tests/test_gpu_rowprog.py: %.1f s since import" % (time.time() - _T0))
