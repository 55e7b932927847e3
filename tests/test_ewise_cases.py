"""CPU checks of tests/ewise_cases.py: the route table reaches every cell it is asked to, each boundary from both sides, in
both element types; the rule of every opcode against numpy; the interpreter against closed forms; the random programs are
not vacuous; the crafted programs need exactly the slots they claim."""
import numpy as np
import pytest

import ewise_cases as E


@pytest.mark.parametrize("dt", E.DTYPES, ids=E.DT_IDS)
def test_every_case_reaches_the_cell_it_names(dt):
    for c in E.route_cases(dt):
        total = E.case_total(c, dt)
        form, blocks, wrap, second = E.ew_plan(dt, c["n"], total, True, None, c["family"])
        assert (form, wrap, second) == (c["form"], c["wrap"], c["second"]), (c["id"], total, form, blocks, wrap, second)
        assert 1 <= blocks <= (1 << 20)
        assert total * np.dtype(dt).itemsize <= (128 << 20) + 16000, c["id"]      # nothing larger than the issue's 128 MiB + 16 KB


@pytest.mark.parametrize("dt", E.DTYPES, ids=E.DT_IDS)
def test_the_table_covers_every_cell(dt):
    have = {(c["family"], c["form"], c["wrap"], c["second"], c["n"]) for c in E.route_cases(dt)}
    for fam, form, wrap, second, n in E.REQUIRED_CELLS:
        if second and fam == "functor" and dt is np.float64:
            continue        # the issue: the functor's second piece in fp32 only
        hit = [h for h in have if h[:4] == (fam, form, wrap, second) and (n is None or h[4] == n)]
        assert hit, (fam, form, wrap, second, n)
    # the VM is scalar whatever the sizes
    assert {c["form"] for c in E.route_cases(dt, "vm")} == {"scalar"}
    # the second piece in fp32 for the functors, in both types for the specialised kernels, there with two inputs as well
    sec = {(c["family"], c["n"]) for c in E.route_cases(dt) if c["second"]}
    assert sec == ({("functor", 1), ("jit", 1), ("jit", 2)} if dt is np.float32 else {("jit", 1), ("jit", 2)})


@pytest.mark.parametrize("dt", E.DTYPES, ids=E.DT_IDS)
@pytest.mark.parametrize("family", ("functor", "jit", "vm"))
def test_each_boundary_has_a_case_on_both_sides(dt, family):
    V = E.vlen(dt)
    totals = {(c["n"], E.case_total(c, dt)) for c in E.route_cases(dt, family)}
    sizes = {t for _, t in totals}
    # scalar wrap: 2048 * 256 threads
    assert any(t <= E.CAP * E.BLOCK and t >= E.CAP * E.BLOCK - 1 for t in sizes) and E.CAP * E.BLOCK + 3 in sizes
    if family == "vm":
        return
    # vec wrap: 2048 * 256 pieces; the streaming threshold: 64 MiB and one piece below; the second piece: 2^23 pieces a trip
    assert V * E.CAP * E.BLOCK in sizes and V * E.CAP * E.BLOCK + V in sizes
    thr = E.STREAM_BYTES // np.dtype(dt).itemsize
    assert thr in sizes and thr - V in sizes
    assert E.ew_plan(dt, 1, thr - V, True, None, family)[0] == "vec" and E.ew_plan(dt, 1, thr, True, None, family)[0] == "stream"
    if family == "jit" or dt is np.float32:
        assert V * ((1 << 23) + 1000) in sizes
        # exactly the first 1000 threads take two pieces
        form, blocks, wrap, second = E.ew_plan(dt, 1, V * ((1 << 23) + 1000), True, None, family)
        assert (form, blocks * E.BLOCK, wrap, second) == ("stream", 1 << 23, False, True)


def test_the_routing_rule_on_alignment_and_periods():
    for dt in E.DTYPES:
        V = E.vlen(dt)
        assert E.ew_plan(dt, 2, 8 * V, False, None, "functor")[0] == "scalar"          # an operand off a 16-byte boundary
        assert E.ew_plan(dt, 2, 8 * V, True, [8 * V, V], "jit")[0] == "vec"            # period % V == 0: the modulo in the vec form
        assert E.ew_plan(dt, 2, 8 * V, True, [8 * V, V + 1], "jit")[0] == "scalar"     # period % V != 0
        assert E.ew_plan(dt, 2, 8 * V, True, [8 * V, 1], "functor")[0] == "scalar"
        assert E.ew_plan(dt, 1, 0, True, None, "functor") == ("scalar", 0, False, False)
        # two inputs: the functors give every thread one piece, the specialised kernels keep the flat cap
        big = V * ((1 << 23) + 1000)
        assert E.ew_plan(dt, 2, big, True, None, "functor")[3] is False and E.ew_plan(dt, 2, big, True, None, "jit")[3] is True
    # the period table reaches both forms in both types
    for dt in E.DTYPES:
        forms = {E.ew_plan(dt, 2, B * n, True, [B * n, n], "functor")[0] for B in E.PERIOD_BATCHES for n in E.PERIOD_NUMELS if B > 1}
        assert forms == {"scalar", "vec"}


# ---- the rules --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", E.DTYPES + (np.longdouble,), ids=E.DT_IDS + ("f80",))
def test_rules_against_numpy(dt):
    """every rule is numpy's function of the same name -- except where the library's rule is NOT numpy's, and there the
    difference is exactly the one DESIGN.md states"""
    base = np.float64 if dt is np.longdouble else dt
    u = E.unary_values(base).astype(dt)
    a, b = (x.astype(dt) for x in E.binary_grid(base))
    def same(x, y):      # values, and the signs of everything that is not a NaN
        ok = ~np.isnan(x)
        return np.array_equal(x, y, equal_nan=True) and np.array_equal(np.signbit(x)[ok], np.signbit(y)[ok])
    with np.errstate(all="ignore"):
        for name, f in (("neg", np.negative), ("exp", np.exp), ("log", np.log), ("sqrt", np.sqrt), ("abs", np.fabs), ("sin", np.sin),
                        ("cos", np.cos), ("tanh", np.tanh), ("recip", np.reciprocal)):
            assert same(E.RULES[E.OPS[name]](u, u), f(u)), name
        for name, f in (("add", np.add), ("sub", np.subtract), ("mul", np.multiply), ("div", np.divide), ("pow", np.power)):
            assert same(E.RULES[E.OPS[name]](a, b), f(a, b)), name
        # signum: numpy's sign but for a zero, which keeps its sign here
        s = E.RULES[E.X_SIGNUM](u, u)
        assert np.array_equal(s, np.sign(u), equal_nan=True)
        z = u == 0
        assert np.array_equal(np.signbit(s[z]), np.signbit(u[z])) and np.signbit(s[z]).any()
        # abs clears the sign of a zero
        assert not np.signbit(E.RULES[E.X_ABS](u, u)[~np.isnan(u)]).any()
        # max / min: numpy's maximum / minimum on ordered pairs of different value ...
        mx, mn = E.RULES[E.X_MAX](a, b), E.RULES[E.X_MIN](a, b)
        ordered = ~np.isnan(a) & ~np.isnan(b)
        assert np.array_equal(mx[ordered], np.maximum(a, b)[ordered]) and np.array_equal(mn[ordered], np.minimum(a, b)[ordered])
        # ... `Ord`'s defaults on the rest: max keeps its first operand, min its second, whichever is the NaN
        un = ~ordered
        assert same(mx[un], a[un]) and same(mn[un], b[un])
        # ... and on equal values (the two zeros) max gives the second operand, min the first
        eq = ordered & (a == b)
        assert same(mx[eq], b[eq]) and same(mn[eq], a[eq])


def test_interpreter_against_closed_forms():
    rng = np.random.default_rng(3)
    x, y = rng.uniform(-3, 3, 500), rng.uniform(-3, 3, 500)
    s = 1 / (1 + np.exp(-y))
    for name, want in (("d_logistic", x * (s * (1 - s))), ("d_tanh", x * (1 - np.tanh(y) ** 2)), ("d_h1mh", x * (y * (1 - y))),
                       ("d_1mh2", x * (1 - y * y)), ("mul", x * y), ("div", x / y)):
        got = E.ssa_eval(E.binary_prog(name), [x, y], np.float64)
        assert np.allclose(np.asarray(got, np.float64), want, rtol=1e-14, atol=1e-14), name
    assert np.allclose(np.asarray(E.ssa_eval(E.unary_prog("logistic"), [y], np.float64), np.float64), s, rtol=1e-15)
    got = E.ssa_eval(E.affine_prog((2.0, -1.0, 0.5, 3.0), 1.0), [x, y, x * y, y - x], np.float64)
    assert np.allclose(np.asarray(got, np.float64), 1 + 2 * x - y + 0.5 * x * y + 3 * (y - x), rtol=1e-14, atol=1e-14)
    for n in (1, 2, 3, 4):
        xs = [rng.integers(-8, 9, 300).astype(np.float64) for _ in range(n)]
        y2 = xs[1] if n >= 2 else 3.0
        want = np.maximum(np.abs(xs[0]) - y2, xs[0] * y2) + y2 - sum(np.abs(t) for t in xs[2:])
        assert np.array_equal(np.asarray(E.ssa_eval(E.piecewise_prog(n), xs, np.float64), np.float64), want)
    # `max r r` is the identity on everything
    u = E.unary_values(np.float64)
    p = E.unary_prog("neg").unclassified()
    got = np.asarray(E.ssa_eval(p, [u], np.float64), np.float64)
    assert np.array_equal(got, -u, equal_nan=True) and np.array_equal(np.signbit(got)[~np.isnan(u)], np.signbit(-u)[~np.isnan(u)])


def test_compare_sees_what_it_should():
    p = E.binary_prog("mul")
    x, y = np.array([1.0, -0.0, 3.0, np.inf], np.float32), np.array([2.0, 5.0, 0.5, 1.0], np.float32)
    good = (x * y).astype(np.float32)
    assert E.compare(good, p, [x, y], np.float32, exact=True, zero_sign=True) is None
    for i, v in ((0, 2.0000002), (1, 0.0), (2, np.nan), (3, -np.inf), (3, 3e38)):
        bad = good.copy()
        bad[i] = v
        assert E.compare(bad, p, [x, y], np.float32, exact=True, zero_sign=True) is not None, (i, v)
    # an intermediate past the element type's range: step by step 0.5 inf - 2 max is inf - inf, the affine functor's fma gives inf
    q = E.affine_prog((0.5, -2.0), 0.0)
    a, b = np.array([np.inf], np.float32), np.array([np.finfo(np.float32).max], np.float32)
    assert E.compare(np.array([np.nan], np.float32), q, [a, b], np.float32) is None
    assert E.compare(np.array([np.inf], np.float32), q, [a, b], np.float32) is not None
    assert E.compare(np.array([np.inf], np.float32), q, [a, b], np.float32, fused=True) is None
    assert E.compare(np.array([-np.inf], np.float32), q, [a, b], np.float32, fused=True) is not None
    bad = good.copy()
    bad[0] = 2.0000002                        # one ulp: inside the band, not exact
    assert E.compare(bad, p, [x, y], np.float32) is None


# ---- the special-value and wide-range tables ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", E.DTYPES, ids=E.DT_IDS)
def test_special_value_tables(dt):
    u = E.unary_values(dt)
    fi = np.finfo(dt)
    for v in (0.0, fi.smallest_subnormal, fi.tiny, 1.0, np.inf, 88.7, 88.8, 103.9, 104.0, 709.7, 709.8, 745.0, 746.0, 110.0, 750.0, 1e-20, 20.0, 1e30):
        for s in (1, -1):
            w = np.asarray(s * v, dtype=dt)
            assert np.any((u == w) & (np.signbit(u) == np.signbit(w))), (s, v)
    assert np.isnan(u).sum() == 1
    a, b = E.binary_grid(dt)
    assert len(E.binary_values(dt)) == 9 and a.size == 81
    # the edges do what they are there for: exp overflows between 88.7 and 88.8 (709.7 and 709.8), underflows to zero between
    # -103.9 and -104 (-745 and -746)
    hi, lo = ((88.7, 88.8), (-103.9, -104.0)) if dt is np.float32 else ((709.7, 709.8), (-745.0, -746.0))
    with np.errstate(all="ignore"):
        e = E.ssa_eval(E.unary_prog("exp"), [np.array(hi + lo, dtype=dt)], dt).astype(dt)
    assert np.isfinite(e[0]) and np.isinf(e[1]) and e[2] > 0 and e[3] == 0


@pytest.mark.parametrize("dt", E.DTYPES, ids=E.DT_IDS)
def test_wide_range_values_stay_in_the_domain(dt):
    for name in ("exp", "logistic", "log", "sqrt", "recip", "tanh", "neg", "abs"):
        x = E.wide_values(name, dt)
        assert x.size == 4096 and np.isfinite(x).all()
        want = E.ssa_eval(E.unary_prog(name), [x], dt).astype(dt)
        assert np.isfinite(want).all(), name
        lo, hi, signed = E.wide_domain(name, dt)
        assert (x < 0).any() == signed and np.log10(float(np.abs(x).max())) - np.log10(float(np.abs(x).min())) > 1.5, name
    for name in ("mul", "div"):
        x, y = E.wide_values(name, dt, seed=1), E.wide_values(name, dt, seed=2)
        assert np.isfinite(E.ssa_eval(E.binary_prog(name), [x, y], dt).astype(dt)).all()
    # the affine sweep reaches |c| / |a| beyond 1e12 and stays finite in fp32
    ratios = [abs(c / a) for c, a in E.affine_sweep()]
    assert max(ratios) > 1e12 and min(ratios) < 1e4
    x = E.affine_sweep_x(dt)
    assert np.abs(x).max() > 1e11 and np.abs(x).min() < 1e-11
    for c, a in E.affine_sweep():
        assert np.isfinite(E.ssa_eval(E.affine_prog((a,), c), [x], dt).astype(dt)).all()


def test_probing_an_affine_program_loses_what_the_issue_says():
    """the emulation behind suspect 1, in double: a = f(1) - f(0) of `1 + 1e-6 x` is off by 8e-11 of itself, and at x = 1e6 the
    functor with that slope is 4e-11 from the program -- past the fp64 tolerance the GPU test applies"""
    c, a, x = E.AFFINE_BY_HAND[0]
    probed = (c + a * 1.0) - c
    assert 1e-11 < abs(probed - a) / a < 1e-9
    want = np.longdouble(c) + np.longdouble(a) * np.longdouble(x)
    assert abs(np.longdouble(c) + np.longdouble(probed) * x - want) / want > 10 * E.TOL[np.float64]


# ---- random programs and the slot limit ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", E.DTYPES, ids=E.DT_IDS)
def test_random_programs_are_not_vacuous(dt):
    progs = E.random_programs(dt)
    assert len(progs) == E.N_RANDOM
    stats = {"twice": 0, "far": 0, "consts": 0, "const_result": 0, "input_result": 0, "long": 0}
    for idx, p in enumerate(progs):
        assert 1 <= p.arity <= 8 and 1 <= len(p.code) <= 200
        for i, (op, a, b) in enumerate(p.code):      # well formed, as to_expr_compile demands
            assert 0 <= op < 18
            assert (0 <= a < len(p.consts)) if op == E.X_CONST else (0 <= a < p.arity + i and 0 <= b < p.arity + i)
        want = E.ssa_eval(p, E.random_inputs(p, dt, idx), dt)
        assert np.isfinite(want).sum() * 2 >= want.size, p.name
        stats["twice"] += any(op != E.X_CONST and a == b and E.OP_NAMES[op] in E.BINARY for op, a, b in p.code)
        stats["far"] += any(op != E.X_CONST and (p.arity + i - min(a, b)) > 20 and min(a, b) >= p.arity for i, (op, a, b) in enumerate(p.code))
        stats["consts"] += sum(op == E.X_CONST for op, a, b in p.code) >= 10
        stats["const_result"] += p.code[-1][0] == E.X_CONST
        stats["input_result"] += p.code[-1][0] == E.X_MAX and p.code[-1][1] == p.code[-1][2] < p.arity
        stats["long"] += len(p.code) >= 100
    assert all(v >= 1 for v in stats.values()), stats
    assert stats["twice"] >= 10 and stats["far"] >= 5 and stats["long"] >= 5, stats
    assert {p.arity for p in progs} >= {1, 8}
    assert max(E.live_slots(p) for p in progs) <= E.slot_cap(dt), "a random program past the VM's slot limit"
    # the same list in every process
    E._PROGRAMS.clear()
    again = E.random_programs(dt)
    assert [(p.arity, p.code, p.consts) for p in again] == [(p.arity, p.code, p.consts) for p in progs]


@pytest.mark.parametrize("dt", E.DTYPES, ids=E.DT_IDS)
def test_slot_programs_need_exactly_k_slots(dt):
    cap = E.slot_cap(dt)
    assert cap == (96 if dt is np.float32 else 48)
    ks = [k for k, _ in E.slot_cases(dt)]
    assert ks[:3] == ([96, 97, 65] if dt is np.float32 else [48, 49, 33])
    for k, runs in E.slot_cases(dt):
        p = E.slots_prog(k)
        assert E.live_slots(p) == k and runs == (k <= cap)
        # 65 fp32 / 33 fp64 slots are the first past 64 KiB of LDS for 256 threads
    assert 64 * 256 * 4 == 65536 and 32 * 256 * 8 == 65536
    x = np.arange(-4, 5, dtype=dt)
    k = 6
    assert np.array_equal(np.asarray(E.ssa_eval(E.slots_prog(k), [x], dt), np.float64), x + 1 - 2 + 3 - 4 + 5)
