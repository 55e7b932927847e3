"""The tables of tests/rowprog_cases.py, checked without a GPU: every program's reference against the oracle's class methods
row by row (and the composite head against the oracle's own TOps and a finite difference), the hand-stated op / constant /
operand / output counts against a count of what the program records, exactness of the exact data in fp32, and the restated
formation rule against a hand-listed expectation at its edges."""
import numpy as np
import pytest

import rowprog_cases as RP
from oracle import neuralnet as NN, top as TO
from oracle.tensor import OTensor

O = OTensor(np.float64)
FINITE = [c for c in RP.ALL_CASES if c["id"] not in ("inf-literals", "nonfinite")]


class RowOracle:
    """the program on ONE row through the oracle's `instance Tensor` (oracle/tensor.py): values are plain numpy arrays"""

    def liftT(self, f, xs):
        return O.liftT(f, xs)

    def gmul(self, lm, lo, ln, x, y):
        return O.gmul(lm, lo, ln, x, y)

    def sumT(self, xs, shape):
        return O.sumT(xs, shape)

    def scaleT(self, alpha, x):
        return O.scaleT(alpha, x)

    def sumRows(self, x):
        return O.sumRows(x)

    def mapRows_const(self, len_n, row, like):
        return O.mapRows(len_n, lambda _r: row, like)

    def konst(self, shape, c):
        return O.konst(shape, c)


def by_rows(case, B, N):
    W, x = RP.root_data(case, B, N)
    ops = RP.operands(case, B, N)
    Wp, s = RP.peer_data(B, N)
    rows = []
    for b in range(B):
        v = {"n": N, "z": O.gmul(1, 1, 0, W, x[b])}
        for name, (kind, a) in ops.items():
            v[name] = np.asarray(a[b] if kind in ("vec_row", "sc_row", "probe") else a)
        if case.get("peer"):
            v["p"] = O.gmul(1, 1, 0, Wp, s[b])
        rows.append([np.asarray(o) for o in case["build"](RowOracle(), v)])
    return [np.stack([r[k] for r in rows]) for k in range(len(rows[0]))]


@pytest.mark.parametrize("case", FINITE, ids=[c["id"] for c in FINITE])
def test_references_are_the_oracles_and_exact(case):
    for B, N in ((RP.OP_B, RP.OP_N), (3, 1024)):
        want, be = RP.reference(case, B, N)
        for w, o in zip(want, by_rows(case, B, N)):
            assert w.shape == o.shape and np.array_equal(w, o), case["id"]
        if case["id"].startswith("dead"):
            continue
        assert be.exact_log() is None, (case["id"], N, be.exact_log())
        for w in want:                       # bit-equal after a round trip through float32
            assert np.array_equal(w.astype(np.float32).astype(np.float64), w)
        w32, _ = RP.reference(case, B, N, work=np.float32)      # ... and evaluated IN float32
        for w, a in zip(want, w32):
            assert np.array_equal(a.astype(np.float64), w)


@pytest.mark.parametrize("case", RP.ALL_CASES, ids=[c["id"] for c in RP.ALL_CASES])
def test_stated_counts_are_what_the_program_records(case):
    for B in (RP.OP_B, 0):
        want, be = RP.reference(case, B, RP.OP_N)
        assert (be.n_ops, be.n_consts, len(want)) == (case["n_ops"], case["n_consts"], case["n_outs"]), case["id"]
        assert len(be.externals) == case["n_ext"], case["id"]
        for w in want:
            assert w.shape[:1] == ((B,) if B else w.shape[:1])


def test_every_row_op_has_a_program_of_its_own():
    ids = {c["id"] for c in RP.OP_CASES}
    assert ids >= {"lift-vec", "lift-vec3", "lift-scalar", "dact-logistic", "dact-tanh", "sum", "scale", "mul", "sum-rows", "dot",
                   "map-rows", "const"}
    assert len({c["id"] for c in RP.ALL_CASES}) == len(RP.ALL_CASES)
    for c in RP.OP_CASES:
        assert RP.forms(RP.OP_N, c["n_ext"], c["n_outs"], c["n_ops"]) and c["n_ops"] <= 4, c["id"]


def test_exact_data_differs_where_a_misplaced_element_would_hide():
    z = RP.x_ints(RP.OP_B) @ RP.w_ints(1024).T
    assert (z[:, 1:] != z[:, :-1]).mean() > 0.8 and (z[:, 64:] != z[:, :-64]).mean() > 0.8          # neighbours, one trip apart
    assert (np.abs(RP.x_ints(130)).sum(axis=1) > 0).all()
    t = RP.UN([z])
    assert (t != 0).all()                     # a dropped term of a row sum or a dot product always shows
    assert RP.probe_columns(65) == [0, 63, 64] and RP.probe_columns(129) == [0, 63, 64, 65, 127, 128]
    assert RP.probe_columns(1024)[-4:] == [959, 960, 961, 1023] and RP.probe_columns(1) == [0]
    for B, N in ((5, 1000), (1, 65), (0, 65)):
        y = RP.probe_targets(B, N)
        assert y.sum() == len(RP.probe_columns(N)) and (y.sum(axis=0) <= 1).all()


def test_saturated_activations_are_exact_in_both_types():
    """logistic(+-800) and tanh(+-800) as the closures compute them: 0, 1/2, 1 and -1, 0, 1 bit for bit"""
    for dt in RP.DTYPES:
        q = np.array([-800.0, 0.0, 800.0], dtype=dt)
        assert np.array_equal(np.asarray(RP.LOGISTIC([q]), dtype=dt), np.array([0.0, 0.5, 1.0], dtype=dt))
        assert np.array_equal(np.asarray(RP.TANH([q]), dtype=dt), np.array([-1.0, 0.0, 1.0], dtype=dt))
    d = np.array([3.0, 3.0, 3.0])
    assert np.array_equal(RP.D_LOGISTIC([d, q]), [0.0, 0.75, 0.0]) and np.array_equal(RP.D_TANH([d, q]), [0.0, 3.0, 0.0])
    want, _ = RP.reference(RP.OP_CASES[3], RP.OP_B, RP.OP_N)
    assert (want[1] == 0.5).mean() > 0.02 and (want[0] != 0).any()       # columns with q = 0 exist: the two forms differ there


def test_dead_lane_cases_are_rows_of_ones():
    for case in RP.DEAD_CASES:
        for N in RP.DEAD_WIDTHS:
            (s, p), _ = RP.reference(case, RP.OP_B, N)
            assert np.array_equal(s, np.full(RP.OP_B, float(N))) and np.array_equal(p, np.full((RP.OP_B, N), 1.0 / N))


def test_non_finite_reference():
    x, clean = RP.poisoned_x(RP.OP_B)
    want, _ = RP.reference(RP.NONFINITE_CASE, RP.OP_B, RP.OP_N, x=x)
    plain, _ = RP.reference(RP.NONFINITE_CASE, RP.OP_B, RP.OP_N)
    for w, p in zip(want, plain):
        for b in range(RP.OP_B):
            assert np.isfinite(w[b]).all() == (b in clean)
            if b in clean:
                assert np.array_equal(w[b], p[b])
    # z itself: a scalar triple loop in IEEE arithmetic
    W = RP.w_ints(RP.OP_N)
    with np.errstate(all="ignore"):
        z = np.array([[sum(W[j, k] * x[b, k] for k in range(RP.K)) for j in range(RP.OP_N)] for b in range(RP.OP_B)])
        s = np.array([sum(-(z[b, j] * z[b, j]) for j in range(RP.OP_N)) for b in range(RP.OP_B)])
    assert RP.same_with_nan(s, want[0])
    assert np.isnan(want[0][1]) and want[0][2] == -np.inf or np.isnan(want[0][2])
    inf, _ = RP.reference(RP.INF_CASE, RP.OP_B, RP.OP_N)
    assert np.isinf(inf[0]).all() and (inf[1] == np.inf).all()
    assert RP.same_with_nan(np.array([np.nan, 1.0]), np.array([np.nan, 1.0])) and not RP.same_with_nan(np.array([0.0, 1.0]), np.array([np.nan, 1.0]))


def test_composite_head_against_the_oracles_tops_and_a_finite_difference():
    rng = np.random.default_rng(0x7e5000b0)
    B, N = 3, 65
    z, y = rng.uniform(-2, 2, (B, N)), rng.uniform(0, 1, (B, N))
    loss, dz = RP.composite_reference(z, y)
    head = TO.first(NN.softmax() >> TO.scale(0.5), 1) >> NN.squaredError()
    for b in range(B):
        assert abs(float(TO.runTOp(head, O, [z[b], y[b]])[0]) - loss[b]) <= 1e-14 * max(1.0, abs(loss[b]))
        g = np.asarray(TO.gradTOp(head, O, [z[b], y[b]])[0])
        assert np.abs(g - dz[b]).max() <= 1e-14
    h = 1e-6
    for j in (0, 17, 64):
        zp, zm = z.copy(), z.copy()
        zp[:, j] += h
        zm[:, j] -= h
        fd = (RP.composite_reference(zp, y)[0] - RP.composite_reference(zm, y)[0]) / (2 * h)
        assert np.abs(fd - dz[:, j]).max() < 1e-8
    lw, dw = RP.composite_reference(z, y, work=np.longdouble)
    assert np.abs(lw - loss).max() < 1e-14 and np.abs(dw - dz).max() < 1e-15


def test_formation_rule_at_its_edges():
    w, e4, e5, o4, o5, p, p5 = (next(c for c in RP.ALL_CASES if c["id"] == i) for i in ("width", "ext-4", "ext-5", "out-4", "out-5", "peer", "peer-5"))
    const = next(c for c in RP.OP_CASES if c["id"] == "const")
    # (launches behind the contractions' own) by hand: a program is 1; none is one per op and constant
    assert [RP.launches(w, N) for N in (1, 64, 65, 1023, 1024, 1025, 2048)] == [1, 1, 1, 1, 1, 4, 4]
    assert RP.launches(w, 1024, rowprog_on=False) == 4
    assert (RP.launches(e4, 65), RP.launches(e5, 65)) == (1, 6)
    assert (RP.launches(o4, 65), RP.launches(o5, 65)) == (1, 6)
    assert (RP.launches(p, 65), RP.launches(p5, 65), RP.launches(p5, 65, rowprog_on=False)) == (1, 2, 6)
    assert RP.launches(p5, 1025) == 6                                     # the retry meets the same width
    assert not RP.forms(0, 0, 1, 2) and RP.forms(1, 0, 1, 2) and not RP.forms(65, 0, 0, 2) and not RP.forms(65, 0, 1, 1)
    assert RP.forms(65, 4, 4, 2) and not RP.forms(65, 5, 4, 2) and not RP.forms(65, 4, 5, 2)
    assert (RP.composite_launches(1024), RP.composite_launches(1025), RP.composite_launches(65, False), RP.composite_launches(1025, False)) == (1, 17, 20, 17)
    assert (RP.composite_elided(65), RP.composite_elided(65, False), RP.composite_elided(1025)) == (18, 0, 3)
    assert (RP.elided(e4, 65), RP.elided(e5, 65), RP.elided(p5, 65), RP.elided(e4, 65, False), RP.elided(const, 65)) == (3, 0, 3, 0, 3)
    assert (RP.launches(const, 65), RP.launches(const, 65, rowprog_on=False)) == (1, 5)
    for c in RP.ALL_CASES:                # formed <=> fewer launches; every case but the two over a limit forms at 65
        assert RP.formed(c, 65) == (c["id"] not in ("ext-5", "out-5")), c["id"]
        assert not RP.formed(c, 1025) and RP.launches(c, 65, rowprog_on=False) > RP.launches(c, 65) - (0 if RP.formed(c, 65) else 1)
    # the compiled programs of the GPU file: distinct (program, N, dtype), at most 80
    n = 0
    for dt in RP.DTYPES:
        n += len(RP.OP_CASES) + 2 * sum(N <= RP.MAX_N for N in RP.widths(dt)) + len(RP.DEAD_CASES) * len(RP.DEAD_WIDTHS)
        n += sum(RP.formed(c, RP.OP_N) for c in RP.EXT_CASES) + 2 + sum(N not in RP.widths(dt) for N in RP.INEXACT_WIDTHS)
    assert n + 1 <= 80, n
