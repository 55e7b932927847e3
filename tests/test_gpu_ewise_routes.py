"""The elementwise kernels behind `to_lift`, route by route and value by value: the three kernel forms (scalar, 16-byte,
streaming) of the pre-fused functors and of the run-time specialised kernels, the bytecode VM, and the entries that go
through `affine_impl`.  Tables, routing restatement and references: tests/ewise_cases.py (checked on the CPU by
tests/test_ewise_cases.py).

 a. values by route: exact data (small integers, dyadic constants: `np.array_equal` over the whole output), every cell of the
    route table, the route asked from the library (`to_ewise_route_query`) and the launch counted; results land in memory
    that held NaN
 b. broadcast periods, unaligned views, `total == 0`, a transposed operand
 c. to_scale / to_sum / to_blas_axpy / to_blas_add / to_sgd_step_inplace
 d. special values and wide ranges per opcode and per functor, through the functor, the specialised kernel and the VM
 e. random SSA programs and the VM's slot limit

The switch TOPS_EXPR_JIT is read once per process: everything that runs on the VM runs in ONE child process (this file, run
as a script), under a time limit of its own; the tests named *_vm read its report."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import ewise_cases as E  # noqa: E402

try:
    import pytest
    pytestmark = pytest.mark.gpu
except ImportError:          # (the child needs none of it)
    pytest = None

NAN = np.nan
_T = {}


def backend(dt):
    from tensor_ops_amd.hipt import HipT
    dt = np.dtype(dt).type
    if dt not in _T:
        _T[dt] = HipT(0, dt)
    return _T[dt]


_EXPRS = {}


def expr(prog):
    from tensor_ops_amd.hipt import Expr
    key = (prog.arity, tuple(prog.code), tuple(float(c).hex() for c in prog.consts))     # (hex: -0.0 and 0.0 are different programs)
    if key not in _EXPRS:
        _EXPRS[key] = Expr(prog.arity, prog.code, prog.consts)
    return _EXPRS[key]


def nan_pool(T, *counts):
    """upload and release NaN-filled tensors of the sizes about to be asked for: the pool memory handed out next is NaN, so an
    element no thread writes shows"""
    held = [T.put(np.full(int(n), NAN, T.dtype.type)) for n in counts if n > 0]
    T.sync()
    del held


def ints(total, i, dt):
    """small integers in [-8, 8], different at neighbouring positions and with a period (17) no piece or trip shares"""
    return ((np.arange(total, dtype=np.int64) * (2 * i + 3) + 5 * i) % 17 - 8).astype(dt)


def dyadic(total, dt):
    """h = k / 8 in [0, 1]"""
    return ((np.arange(total, dtype=np.int64) * 5 % 9) / 8.0).astype(dt)


def lift(T, prog, ops, family, kind=None, extra_launches=0, expect=None, fails=None, ctx=""):
    """one to_lift of `prog` over device operands `ops`: the kind, the route (restated, asked from the library, and the table's
    if given), the launch count; returns the result as numpy"""
    fails = fails if fails is not None else []
    e = expr(prog)
    want_kind = kind if kind is not None else E.KIND[family]
    if e.kind != want_kind:
        fails.append("%s %s: kind %d, expected %d" % (ctx, prog.name, e.kind, want_kind))
    B = max(o.batch for o in ops)
    numel = int(np.prod(ops[0].shape)) if len(ops[0].shape) else 1
    total = max(B, 1) * numel
    periods = [total if (o.batch > 0 or B == 0) else max(numel, 1) for o in ops]
    aligned = all(o.ptr % 16 == 0 for o in ops) if extra_launches == 0 else True
    plan = E.ew_plan(T.dtype, len(ops), total, aligned, periods, family)
    got_route = T.ewise_route(total, len(ops), family, periods if total else None, aligned)
    if got_route != (plan[0], plan[1], plan[3]):
        fails.append("%s %s: the library routes %s, the restatement %s" % (ctx, prog.name, got_route, plan))
    if expect is not None and (plan[0], plan[2], plan[3]) != expect:
        fails.append("%s %s: reaches %s, the table says %s" % (ctx, prog.name, (plan[0], plan[2], plan[3]), expect))
    nan_pool(T, total)
    before = T.stats()["launches"]
    out = T.liftT(e, ops)
    launched = T.stats()["launches"] - before
    if launched != (1 if total else 0) + extra_launches:
        fails.append("%s %s: %d launches, expected %d" % (ctx, prog.name, launched, (1 if total else 0) + extra_launches))
    if total and out.ptr % 16:
        fails.append("%s: a fresh result off a 16-byte boundary" % ctx)
    return out.numpy()


def exact(got, prog, xs, dt, fails, ctx):
    want = np.asarray(E.ssa_eval(prog, xs, dt, work=np.dtype(dt).type))
    if got.shape != want.shape or not np.array_equal(got, want):
        bad = np.flatnonzero(got.ravel() != want.ravel())[:5] if got.shape == want.shape else []
        fails.append("%s %s: %s" % (ctx, prog.name, [(int(i), float(want.ravel()[i]), float(got.ravel()[i])) for i in bad] or (got.shape, want.shape)))


# programs of the exact tests: (program, kind) by family and arity
AFF = {1: E.affine_prog((2.0,), 1.0), 2: E.affine_prog((2.0, -1.0), 1.0), 3: E.affine_prog((2.0, -1.0, 0.5), 1.0),
       4: E.affine_prog((2.0, -1.0, 0.5, 3.0), -1.5)}


def route_programs(family, n):
    if family == "functor":
        return [(AFF[n], 1)] + ([(E.binary_prog("mul"), 2)] if n == 2 else [])
    return [(E.piecewise_prog(n), E.KIND[family])]


def run_route_case(case, dt, fails):
    T = backend(dt)
    total = E.case_total(case, dt)
    xs = [ints(total, i, dt) for i in range(case["n"])]
    ops = [T.put(x) for x in xs]
    for prog, kind in route_programs(case["family"], case["n"]):
        got = lift(T, prog, ops, case["family"], kind, expect=(case["form"], case["wrap"], case["second"]), fails=fails, ctx=case["id"])
        exact(got, prog, xs, dt, fails, case["id"])
    if case["n"] == 2 and case["family"] != "functor" and total < (1 << 22):        # d * h (1 - h) on dyadic h
        h = dyadic(total, dt)
        prog = E.binary_prog("d_h1mh")
        got = lift(T, prog, [ops[0], T.put(h)], case["family"], fails=fails, ctx=case["id"])
        exact(got, prog, [xs[0], h], dt, fails, case["id"])


def run_period_cases(dt, family, fails):
    """batched operands of B samples mixed with unbatched ones of numel elements: period % V != 0 takes the scalar form,
    period % V == 0 the 16-byte form with the modulo; B = 1 beside an unbatched operand; all operands batched"""
    T = backend(dt)
    two = AFF[2] if family == "functor" else E.piecewise_prog(2)
    three = AFF[3] if family == "functor" else E.piecewise_prog(3)
    kind = 1 if family == "functor" else E.KIND[family]
    for B in E.PERIOD_BATCHES:
        for numel in E.PERIOD_NUMELS:
            ctx = "%s B%d x %d" % (family, B, numel)
            xb = [ints(B * numel, i, dt).reshape(B, numel) for i in range(3)]
            xu = [ints(numel, 3 + i, dt) for i in range(2)]
            db, du = [T.put(x, batched=True) for x in xb], [T.put(x) for x in xu]
            bc = [np.broadcast_to(x, (B, numel)) for x in xu]
            for ops, host in (((db[0], du[0]), (xb[0], bc[0])), ((du[0], db[0]), (bc[0], xb[0])), ((db[0], db[1]), (xb[0], xb[1]))):
                got = lift(T, two, list(ops), family, kind, fails=fails, ctx=ctx)
                exact(got, two, list(host), dt, fails, ctx)
            for ops, host in (((du[0], db[0], du[1]), (bc[0], xb[0], bc[1])), ((db[0], db[1], db[2]), (xb[0], xb[1], xb[2]))):
                got = lift(T, three, list(ops), family, kind, fails=fails, ctx=ctx)
                exact(got, three, list(host), dt, fails, ctx)


def run_unaligned_cases(dt, family, fails):
    """contiguous views that start 1, 2, 3 elements (fp32) or 1 element (fp64) into a buffer with NaN on both sides, as the
    first operand and as the second: the scalar form, correct values"""
    from tensor_ops_amd.hipb import HipB
    T = backend(dt)
    Bl = HipB(0, dtype=dt)
    V = E.vlen(dt)
    prog = (E.binary_prog("mul") if family == "functor" else E.piecewise_prog(2))
    kind = 2 if family == "functor" else E.KIND[family]
    for off in range(1, V):
        # (a) to_batch_slice: `off` samples of one element in, 4 V samples long -- the size alone would vectorise
        count = 4 * V
        x = ints(count, 0, dt)
        big = np.full((off + count + 3, 1), NAN, dtype=dt)
        big[off:off + count, 0] = x
        view = T.batch_slice(T.put(big, batched=True), off, count)
        y = ints(count, 1, dt)
        for first in (True, False):
            ops = [view, T.put(y.reshape(count, 1), batched=True)]
            host = [x.reshape(count, 1), y.reshape(count, 1)]
            if not first:
                ops.reverse()
                host.reverse()
            assert view.ptr % 16 == off * np.dtype(dt).itemsize
            assert family == "vm" or E.ew_plan(dt, 2, count, True, None, family)[0] == "vec"      # only the offset makes it scalar
            got = lift(T, prog, ops, family, kind, fails=fails, ctx="batch_slice+%d" % off)
            exact(got, prog, host, dt, fails, "batch_slice+%d first=%s" % (off, first))
        # (b) to_slice and to_blas_index_row: row 1 of a [3, n] matrix, n = off (mod V), rows 0 and 2 NaN
        n = 25 * V + off
        m = np.full((3, n), NAN, dtype=dt)
        m[1] = ints(n, 2, dt)
        dm = T.put(m)
        y = ints(n, 3, dt)
        for name, view in (("slice", T.slice(dm, (1,))), ("index_row", Bl.indexRowB(1, dm))):
            assert view.ptr % 16 == (n * np.dtype(dt).itemsize) % 16 != 0
            for first in (True, False):
                ops, host = [view, T.put(y)], [m[1], y]
                if not first:
                    ops.reverse()
                    host.reverse()
                got = lift(T, prog, ops, family, kind, fails=fails, ctx="%s+%d" % (name, off))
                exact(got, prog, host, dt, fails, "%s+%d first=%s" % (name, off, first))


# ---- special values, wide ranges, random programs: shared by the parent (functor, specialised kernel) and the child (VM) ----------
def valued(T, prog, xs, family, fails, ctx, kind=None, exact_op=False, zero_sign=False):
    got = lift(T, prog, [T.put(x) for x in xs], family, kind, fails=fails, ctx=ctx)
    msg = E.compare(got, prog, xs, T.dtype.type, exact=exact_op, zero_sign=zero_sign, fused=family == "functor" and kind == 1)
    if msg:
        fails.append("%s [%s]: %s" % (ctx, family, msg))


def evaluators(prog, functor_kind, vm):
    """(program, family, kind): as written (a functor where the classifier knows one) and behind `max r r`, which no
    classifier touches; in the child everything unclassified is the VM's"""
    other = "vm" if vm else "jit"
    wrapped = (prog.unclassified(), other, E.KIND[other])
    if functor_kind is not None:
        return [(prog, "functor", functor_kind), wrapped]
    return [(prog, other, E.KIND[other]), wrapped]


UNARY_KIND = {"logistic": 6, "exp": 3, "log": 4, "recip": 5, "tanh": 8, "sqrt": 9, "neg": 1}
BINARY_KIND = {"mul": 2, "div": 10, "d_logistic": 7, "d_tanh": 13, "add": 1, "sub": 1}


def run_specials(dt, vm, fails, groups=("unary", "binary")):
    T = backend(dt)
    u = E.unary_values(dt)
    for name in (E.UNARY + ("logistic",) if "unary" in groups else ()):
        for prog, family, kind in evaluators(E.unary_prog(name), UNARY_KIND.get(name), vm):
            # (an affine functor does not keep the sign of a zero sum: DESIGN.md; `neg` is fma(-1, x, -0), which does)
            valued(T, prog, [u], family, fails, "special " + name, kind, exact_op=name in E.EXACT_OPS, zero_sign=name in E.ZERO_SIGN_OPS)
    a, b = E.binary_grid(dt)
    if "binary" not in groups:
        return
    for name in E.BINARY + E.FUNCTOR_BINARY[2:] + E.PLANNER_BINARY:
        for prog, family, kind in evaluators(E.binary_prog(name), BINARY_KIND.get(name), vm):
            valued(T, prog, [a, b], family, fails, "special " + name, kind, exact_op=name in E.EXACT_OPS,
                   zero_sign=name in E.ZERO_SIGN_OPS and kind != 1)
    for coefs, c in (((2.0,), 1.0), ((3.0,), None), ((0.5, -2.0), 0.0)):        # affine: no zero signs
        prog = E.affine_prog(coefs, c)
        xs = [u] if len(coefs) == 1 else [a, b]
        for p, family, kind in evaluators(prog, 1, vm):
            valued(T, p, xs, family, fails, "special affine %s %s" % (coefs, c), kind)


def run_wide(dt, vm, fails):
    T = backend(dt)
    for name in ("exp", "logistic", "log", "sqrt", "recip", "tanh", "neg", "abs"):
        x = E.wide_values(name, dt)
        for prog, family, kind in evaluators(E.unary_prog(name), UNARY_KIND.get(name), vm):
            valued(T, prog, [x], family, fails, "wide " + name, kind, exact_op=name in E.EXACT_OPS, zero_sign=name in E.ZERO_SIGN_OPS)
    for name in ("mul", "div"):
        x, y = E.wide_values(name, dt, seed=1), E.wide_values(name, dt, seed=2)
        for prog, family, kind in evaluators(E.binary_prog(name), BINARY_KIND[name], vm):
            valued(T, prog, [x, y], family, fails, "wide " + name, kind, exact_op=True, zero_sign=True)


def run_affine_by_hand(dt, vm, fails):
    """`c + a x` with |c| >> |a| at large x: the slope has to be the one the program was written with"""
    T = backend(dt)
    for c, a, x0 in E.AFFINE_BY_HAND:
        x = np.array([x0, -x0, x0 / 3, 1.0, 0.0, 7 * x0 / 8], dtype=dt)
        for prog, family, kind in evaluators(E.affine_prog((a,), c), 1, vm):
            valued(T, prog, [x], family, fails, "affine %g + %g x at %g" % (c, a, x0), kind)


def run_affine_sweep(dt, fails):
    T = backend(dt)
    x = E.affine_sweep_x(dt)
    for c, a in E.affine_sweep():
        valued(T, E.affine_prog((a,), c), [x], "functor", fails, "affine sweep %g + %g x" % (c, a), 1)
    x2 = E.affine_sweep_x(dt, seed=8)
    for (c, a), (_, a2) in zip(E.affine_sweep()[:6], E.affine_sweep(seed=9)[:6]):
        valued(T, E.affine_prog((a, a2), c), [x, x2], "functor", fails, "affine sweep %g + %g x + %g y" % (c, a, a2), 1)


def run_random(dt, vm, fails, chunk=None):
    T = backend(dt)
    family = "vm" if vm else "jit"
    for idx, prog in enumerate(E.random_programs(dt)):
        if chunk is not None and idx % 4 != chunk:
            continue
        e = expr(prog)
        fam, kind = (family, E.KIND[family]) if e.kind in (0, 100) else ("functor", e.kind)     # (a short program may be a functor's)
        valued(T, prog, E.random_inputs(prog, dt, idx), fam, fails, prog.name, kind)


def run_slots(dt, fails):
    """VM only: k simultaneously live values at the cap, one past it, and the first size past 64 KiB of LDS"""
    from tensor_ops_amd.capi import TensorOpsError
    T = backend(dt)
    x = np.arange(-500, 500, dtype=dt)
    for k, runs in E.slot_cases(dt):
        prog = E.slots_prog(k).unclassified()        # (`x + constant` would be an affine functor's)
        try:
            got = lift(T, prog, [T.put(x)], "vm", fails=fails, ctx="slots %d" % k)
            if not runs:
                fails.append("slots %d: ran, expected TO_ERR_UNSUPPORTED" % k)
            else:
                exact(got, prog, [x], dt, fails, "slots %d" % k)
        except TensorOpsError as err:
            if runs or err.code != 5 or "too many live values" not in str(err):
                fails.append("slots %d: %s" % (k, err))


# ---- the child: everything the VM runs ---------------------------------------------------------------------------------------------
def vm_child():
    report = {}
    for dt, name in zip(E.DTYPES, E.DT_IDS):
        for section, fn in (("routes", lambda f: [run_route_case(c, dt, f) for c in E.route_cases(dt, "vm")]),
                            ("periods", lambda f: run_period_cases(dt, "vm", f)),
                            ("unaligned", lambda f: run_unaligned_cases(dt, "vm", f)),
                            ("specials", lambda f: run_specials(dt, True, f)),
                            ("wide", lambda f: (run_wide(dt, True, f), run_affine_by_hand(dt, True, f))),
                            ("random", lambda f: run_random(dt, True, f)),
                            ("slots", lambda f: run_slots(dt, f))):
            fails = []
            try:
                fn(fails)
            except Exception as err:  # noqa: BLE001
                fails.append("exception: %r" % (err,))
            report["%s-%s" % (section, name)] = fails[:12]
    print("VMREPORT " + json.dumps(report))


if __name__ == "__main__":
    vm_child()
    sys.exit(0)


@pytest.fixture(scope="module")
def vm_report():
    env = dict(os.environ, TOPS_EXPR_JIT="0", PYTHONPATH=ROOT)
    out = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, cwd=ROOT)
    if out.returncode < 0 or out.returncode in (124, 134, 137, 139):      # a fault or a hang: nothing more on this device
        pytest.exit("the VM child ended with %d: %s" % (out.returncode, (out.stdout + out.stderr)[-1500:]), returncode=3)
    line = [l for l in out.stdout.splitlines() if l.startswith("VMREPORT ")]
    assert out.returncode == 0 and line, out.stdout[-2000:] + out.stderr[-2000:]
    return json.loads(line[-1][len("VMREPORT "):])


DT = pytest.mark.parametrize("dt", E.DTYPES, ids=E.DT_IDS)


# ---- a. values by route -------------------------------------------------------------------------------------------------------------
def _route_params():
    return [pytest.param(c, dt, id="%s-%s" % (c["id"], n)) for dt, n in zip(E.DTYPES, E.DT_IDS) for c in E.route_cases(dt) if c["family"] != "vm"]


@pytest.mark.parametrize("case,dt", _route_params())
def test_values_by_route(case, dt):
    fails = []
    run_route_case(case, dt, fails)
    assert not fails, fails


@DT
@pytest.mark.parametrize("section", ("routes", "periods", "unaligned"))
def test_values_by_route_vm(vm_report, section, dt):
    key = "%s-%s" % (section, E.DT_IDS[E.DTYPES.index(dt)])
    assert vm_report[key] == [], vm_report[key]


@DT
def test_affine_arity_3_and_4(dt):
    T = backend(dt)
    V = E.vlen(dt)
    fails = []
    for total in (1003, V * 1000, E.CAP * E.BLOCK + 3, V * E.CAP * E.BLOCK + V):
        xs = [ints(total, i, dt) for i in range(4)]
        ops = [T.put(x) for x in xs]
        for n in (3, 4):
            got = lift(T, AFF[n], ops[:n], "functor", 1, fails=fails, ctx="total %d" % total)
            exact(got, AFF[n], xs[:n], dt, fails, "total %d" % total)
    assert not fails, fails


# ---- b. periods, views, empty, transposed ---------------------------------------------------------------------------------------------
@DT
@pytest.mark.parametrize("family", ("functor", "jit"))
def test_broadcast_periods(dt, family):
    fails = []
    run_period_cases(dt, family, fails)
    assert not fails, fails[:10]


@DT
def test_stream_form_under_a_4096_element_period(dt):
    """a 64 MiB batched operand over an unbatched one of 4096 elements: the streaming kernel's modulo"""
    T = backend(dt)
    numel = 4096
    B = E.STREAM_BYTES // np.dtype(dt).itemsize // numel
    xb, xu = ints(B * numel, 0, dt).reshape(B, numel), ints(numel, 1, dt)
    fails = []
    for prog, family, kind in ((AFF[2], "functor", 1), (E.piecewise_prog(2), "jit", 100)):
        got = lift(T, prog, [T.put(xb, batched=True), T.put(xu)], family, kind, expect=("stream", False, False), fails=fails, ctx="period 4096")
        exact(got, prog, [xb, np.broadcast_to(xu, xb.shape)], dt, fails, "period 4096")
    assert not fails, fails


@DT
@pytest.mark.parametrize("family", ("functor", "jit"))
def test_unaligned_views(dt, family):
    fails = []
    run_unaligned_cases(dt, family, fails)
    assert not fails, fails[:10]


@DT
def test_empty_and_transposed_operands(dt):
    T = backend(dt)
    fails = []
    z = np.zeros((0, 5), dtype=dt)
    for prog, family, kind in ((AFF[2], "functor", 1), (E.piecewise_prog(2), "jit", 100)):
        got = lift(T, prog, [T.put(z), T.put(z)], family, kind, fails=fails, ctx="empty")        # no launch: lift counts
        assert got.shape == (0, 5)
        a, b = ints(35, 0, dt).reshape(5, 7), ints(35, 1, dt).reshape(7, 5)
        # one more launch for every operand `contiguous()` has to pack
        got = lift(T, prog, [T.transp(T.put(a)), T.put(b)], family, kind, extra_launches=1, fails=fails, ctx="transposed first")
        exact(got, prog, [a.T, b], dt, fails, "transposed first")
        got = lift(T, prog, [T.transp(T.put(a)), T.transp(T.put(b.T.copy()))], family, kind, extra_launches=2, fails=fails, ctx="transposed both")
        exact(got, prog, [a.T, b], dt, fails, "transposed both")
    assert not fails, fails


# ---- c. the entries through affine_impl -----------------------------------------------------------------------------------------------
@DT
def test_scale_axpy_add(dt):
    from tensor_ops_amd.hipb import HipB
    T, Bl = backend(dt), HipB(0, dtype=dt)
    V = E.vlen(dt)
    for total in (1003, V * E.CAP * E.BLOCK + V, E.CAP * E.BLOCK + 3):
        x, y = ints(total, 0, dt), ints(total, 1, dt)
        dx, dy = T.put(x), T.put(y)
        for name, f, want, n in (("scale", lambda: T.scaleT(-1.5, dx), -1.5 * x, 1), ("axpy", lambda: Bl.axpy(0.5, dx, dy), 0.5 * x + y, 2),
                                 ("axpy-", lambda: Bl.axpy(-3.0, dx, None), -3.0 * x, 1), ("add", lambda: Bl.addB(dx, dy), x + y, 2)):
            nan_pool(T, total)
            before = T.stats()["launches"]
            got = f()
            assert T.stats()["launches"] - before == 1, (name, total)
            assert np.array_equal(got.numpy(), want.astype(dt)), (name, total)
    # a period: scaleT of a batched operand is full-size; sumT / axpy below mix
    B, numel = 3, 6
    xb, xu = ints(B * numel, 0, dt).reshape(B, numel), ints(numel, 1, dt)
    assert np.array_equal(T.scaleT(2.0, T.put(xb, batched=True)).numpy(), 2 * xb)
    # the sign of a zero: an affine functor is fma(a, x, +0) -- scaleT of -0.0 is +0.0
    got = T.scaleT(2.0, T.put(np.array([-0.0, 0.0, -1.0], dtype=dt))).numpy()
    assert np.array_equal(got, [0.0, 0.0, -2.0]) and not np.signbit(got[:2]).any()


@DT
def test_sum_is_a_left_fold_in_groups_of_four(dt):
    """n = 0 .. 9 terms, batched and unbatched mixed, integers: the value, and 0 / 0 / 1 / 1 / 1 / 2 / 2 / 2 / 3 / 3 launches"""
    T = backend(dt)
    B, numel = 3, 6
    terms, host = [], []
    for i in range(9):
        if i % 3 == 1:
            x = ints(numel, i, dt)
            terms.append(T.put(x))
            host.append(np.broadcast_to(x, (B, numel)))
        else:
            x = ints(B * numel, i, dt).reshape(B, numel)
            terms.append(T.put(x, batched=True))
            host.append(x)
    for n in range(10):
        nan_pool(T, B * numel)
        before = T.stats()["launches"]
        got = T.sumT(terms[:n], (numel,))
        launched = T.stats()["launches"] - before
        if n == 0:
            assert np.array_equal(got.numpy(), np.zeros(numel, dtype=dt))
            continue
        if n == 1:           # sumT [x] = x: the same handle
            assert np.array_equal(got.numpy(), host[0]) and launched == 0
            continue
        acc = np.array(host[0], dtype=dt)
        for h in host[1:n]:
            acc = acc + h
        assert np.array_equal(got.numpy(), acc), n
        assert launched == (n + 1) // 3, (n, launched)
    # the grouping shows where rounding does: (((1 + e) + e) + e) + e with e = half an ulp stays 1 term by term; the functor adds
    # four terms with one rounding each in the same order: fma(1, x3, fma(1, x2, fma(1, x1, x0)))
    eps = np.finfo(dt).eps
    vals = [1.0] + [eps / 2] * 8
    ts = [T.put(np.full(5, v, dtype=dt)) for v in vals]
    got = T.sumT(ts, (5,)).numpy()
    acc = np.asarray(vals[0], dtype=dt)
    for v in vals[1:]:
        acc = (acc + np.asarray(v, dtype=dt)).astype(dt)
    assert np.array_equal(got, np.full(5, acc, dtype=dt)), (got[0], acc)       # left to right: every eps/2 is lost; right to left gives 1 + 4 eps
    # one wrap size
    total = E.CAP * E.BLOCK + 3
    xs = [ints(total, i, dt) for i in range(5)]
    got = T.sumT([T.put(x) for x in xs], (total,)).numpy()
    assert np.array_equal(got, sum(xs[1:], xs[0]))


@DT
def test_sgd_step_in_place(dt):
    """p <- p - rate g over 2048 * 256 + 5 elements (the grid-stride wrap), in place, inside a larger buffer whose other
    elements stay as they were"""
    from tensor_ops_amd.capi import check, lib
    T = backend(dt)
    n, pad = E.CAP * E.BLOCK + 5, 7
    p0, g = ints(n, 0, dt), ints(n, 1, dt)
    parent = np.full((pad + n + pad, 1), 99.0, dtype=dt)
    parent[pad:pad + n, 0] = p0
    dparent = T.put(parent, batched=True)
    view = T.batch_slice(dparent, pad, n)
    dg = T.put(g.reshape(n, 1), batched=True)
    before = T.stats()["launches"]
    check(lib().to_sgd_step_inplace(view.h, dg.h, 0.5))
    assert T.stats()["launches"] - before == 1
    want = parent.copy()
    want[pad:pad + n, 0] = p0 - 0.5 * g
    assert np.array_equal(dparent.numpy(), want)
    assert np.array_equal(view.numpy()[:, 0], p0 - 0.5 * g)


# ---- d. special values and wide ranges --------------------------------------------------------------------------------------------------
@DT
@pytest.mark.parametrize("group", ("unary", "binary"))
def test_special_values(dt, group):
    fails = []
    run_specials(dt, False, fails, (group,))
    assert not fails, fails[:10]


@DT
def test_wide_ranges(dt):
    fails = []
    run_wide(dt, False, fails)
    assert not fails, fails[:10]


@DT
def test_affine_programs_by_hand(dt):
    """1 + 1e-6 x at 1e6, 100 + 0.001 x at 1e5, 1e8 + 1e-8 x at 1e12: a slope recovered by probing the program loses
    |c| / |a| of its digits"""
    fails = []
    run_affine_by_hand(dt, False, fails)
    assert not fails, fails


@DT
def test_affine_sweep(dt):
    fails = []
    run_affine_sweep(dt, fails)
    assert not fails, fails[:10]


def test_host_evaluator_folds_constants_by_the_same_rules():
    """`expr_eval` (csrc/expr.cpp) is reachable through the ABI where the classifier folds a constant program: `op k1 k2`
    compiles to the affine functor 0 x + c with c = the host's value of the op.  At x = -1 the functor returns c bit for
    bit (0 * -1 + c keeps either zero), so the host's value of every exact smooth opcode, the two zeros and a denormal
    included, shows in the result: it has to be the rule of the table, which the device evaluators are held to above.  (abs,
    signum, max and min are never classified, so the host never evaluates them for a result.)"""
    T = backend(np.float64)
    fi = np.finfo(np.float64)
    vals = (0.0, -0.0, 1.0, -2.5, float(fi.smallest_subnormal))
    x = T.put(np.array([-1.0]))
    fails = []
    cases = [(n, a, a) for n in ("neg", "recip", "sqrt") for a in vals]
    cases += [(n, a, b) for n in ("add", "sub", "mul", "div") for a in vals for b in vals]
    for name, a, b in cases:
        with np.errstate(all="ignore"):
            want = np.float64(E.RULES[E.OPS[name]](np.array([a]), np.array([b]))[0])
        if not np.isfinite(want):
            continue            # (no constant to fold: the program is not affine and runs as written)
        p = E.Prog(1, "const-" + name)
        p.op(name, p.k(a), p.k(b))
        e = expr(p)
        got = T.liftT(e, [x]).numpy()[0]
        if e.kind != 1 or got != want or np.signbit(got) != np.signbit(want):
            fails.append((name, a, b, e.kind, float(want), float(got)))
    assert not fails, fails[:8]


@DT
@pytest.mark.parametrize("section", ("specials", "wide"))
def test_special_values_and_wide_ranges_vm(vm_report, section, dt):
    key = "%s-%s" % (section, E.DT_IDS[E.DTYPES.index(dt)])
    assert vm_report[key] == [], vm_report[key]


# ---- e. random programs, the slot limit -------------------------------------------------------------------------------------------------
@DT
@pytest.mark.parametrize("chunk", range(4))
def test_random_programs(dt, chunk):
    """40 programs a type, ten a test: each is compiled by hiprtc for fp32 (to_expr_kind) and for the type it runs in"""
    fails = []
    run_random(dt, False, fails, chunk)
    assert not fails, fails[:10]


@DT
@pytest.mark.parametrize("section", ("random", "slots"))
def test_random_programs_and_slot_limit_vm(vm_report, section, dt):
    key = "%s-%s" % (section, E.DT_IDS[E.DTYPES.index(dt)])
    assert vm_report[key] == [], vm_report[key]


def test_route_query_refuses_bad_arguments():
    from tensor_ops_amd.capi import TensorOpsError
    T = backend(np.float32)
    assert T.ewise_route(0, 1) == ("scalar", 0, False)
    for kw in (dict(total=-1, n_inputs=1), dict(total=8, n_inputs=9), dict(total=8, n_inputs=1, periods=[0]), dict(total=8, n_inputs=1, periods=[9])):
        with pytest.raises(TensorOpsError) as ei:
            T.ewise_route(**kw)
        assert ei.value.code == 1
