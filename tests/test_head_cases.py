"""The tables and the reference of tests/head_cases.py, checked without a GPU: the lse form of the loss is the literal
-y log softmax(z) wherever that one is finite, every case has the property it was built for, the special rows have the
classes the table says, and the finite cases cover every width."""
import numpy as np
import pytest

import head_cases as HC

IDS = ["f32", "f64"]
ALL_WIDTHS = sorted({n for ws in HC.WIDTHS.values() for n in ws})


@pytest.mark.parametrize("dt", HC.DTYPES, ids=IDS)
def test_the_lse_reference_is_the_literal_loss_where_that_is_finite(dt):
    seen_finite = seen_not = 0
    for n in ALL_WIDTHS:
        for c in HC.finite_cases(n, dt):
            _, _, loss = HC.softmax_ce(c["z"], c["y"])
            lit = HC.softmax_ce_literal(c["z"], c["y"])
            assert np.isfinite(loss), c["id"]
            if np.isfinite(lit):
                seen_finite += 1
                assert abs(loss - lit) <= 1e-12 * max(1.0, abs(lit)), (c["id"], loss, lit)
            else:
                seen_not += 1
                assert c["spread"] > HC.EXP_RANGE[np.float64], c["id"]      # only float64's own underflow gets here
    assert seen_finite and seen_not


@pytest.mark.parametrize("dt", HC.DTYPES, ids=IDS)
def test_every_case_has_the_property_it_was_built_for(dt):
    for n in ALL_WIDTHS:
        cases = HC.finite_cases(n, dt)
        assert len(cases) == len(HC.SPREADS) * len(HC.PATTERNS) * len(HC.TARGETS)
        assert len({c["id"] for c in cases}) == len(cases)
        for c in cases:
            z, y = c["z"], c["y"]
            # exact in the element type, z - max finite, the target's sum exact
            assert np.array_equal(HC.stored(z, dt), z) and np.array_equal(HC.stored(y, dt), y), c["id"]
            assert np.isfinite(z - z.max()).all() and np.isfinite(HC.stored(z - z.max(), np.float32)).all(), c["id"]
            assert y.sum() == HC.TARGET_SUM[c["target"]] and (y >= 0).all(), c["id"]
            assert float(np.asarray(y, dt).sum(dtype=dt)) == HC.TARGET_SUM[c["target"]], c["id"]
            if c["target"].startswith("soft"):
                assert (y > 0).all(), c["id"]
            # the spread is the nominal one wherever the pattern has two different logits, and on the side of the element
            # type's range the table says
            flat = c["pattern"] == "equal" or n == 1 or (c["pattern"] == "two_max" and n == 2)
            want = 0.0 if flat else float(HC.stored(0.5 * c["nominal"], dt)) * 2
            assert c["spread"] == want, (c["id"], c["spread"], want)
            assert c["underflow"] == (not flat and c["nominal"] > (100.0 if dt == np.float32 else 120.0)), c["id"]
            p, dz, loss = HC.softmax_ce(z, y)
            assert np.isfinite(p).all() and np.isfinite(dz).all() and np.isfinite(loss), c["id"]
            assert (p.min() == 0.0) == (c["spread"] > HC.EXP_RANGE[np.float64]), c["id"]
            # the earliest-index rule has something to decide exactly where the table says
            # (the ramp repeats from logit 9 on: its largest value comes a second time at logit 17)
            unique_max = n == 1 or (c["nominal"] > 0 and (c["pattern"] == "dominant" or (c["pattern"] == "ramp" and n < 18)))
            assert c["tie_free"] == unique_max, c["id"]
        # every batch, the one of a single row too, has a cotangent far from zero: a relative bound on its gradients means
        # something (one logit: dz = sum(y) - y = 0 whatever the row)
        for b in HC.batches(cases):
            _, dz, _ = HC.softmax_ce(np.stack([c["z"] for c in b]), np.stack([c["y"] for c in b]))
            assert n == 1 or np.abs(dz).max() >= 0.25, [c["id"] for c in b]
        assert sorted({len(b) for b in HC.batches(cases)}) == [1, 5, 7]


@pytest.mark.parametrize("dt", HC.DTYPES, ids=IDS)
def test_the_special_rows_have_the_classes_the_table_says(dt):
    for n in ALL_WIDTHS:
        sp = HC.special_batches(n, dt)
        assert {c["id"].split("-")[0] for c in sp} == {"nan_logit", "pinf_logit", "all_ninf", "nan_target"} | ({"ninf_logit"} if n >= 2 else set())
        for c in sp:
            assert np.isfinite(c["x"]).all(), c["id"]          # never in x: a contraction would spread it over the row
            p, dz, loss = HC.softmax_ce(c["x"] + c["bias"], c["y"])
            assert list(HC.klass(loss)) == c["loss_class"], (c["id"], loss)
            kind = c["id"].split("-")[0]
            if kind in ("nan_logit", "pinf_logit", "all_ninf"):
                assert np.isnan(p).all() and np.isnan(dz).all(), c["id"]
            elif kind == "ninf_logit":
                assert np.isfinite(p).all() and np.isfinite(dz).all() and (p[:, n // 2] == 0).all(), c["id"]
            else:
                assert np.isfinite(p).all() and np.isnan(dz[3]).all() and np.isfinite(np.delete(dz, 3, axis=0)).all(), c["id"]


def test_the_squared_error_references_are_the_formulas_of_the_head():
    z = np.array([[-1000.0, -2.0, 0.0, 0.5, 1000.0]])
    t = np.array([[0.0, 0.25, 1.0, 0.5, 1.0]])
    a, dz, loss = HC.logistic_se(z, t)
    assert np.array_equal(a[0, [0, 2, 4]], [0.0, 0.5, 1.0]) and np.isfinite(dz).all()
    assert np.allclose(dz, 2 * (a - t) * a * (1 - a), rtol=1e-15, atol=0) and loss[0] == ((a - t) ** 2).sum()
    a, dz, _ = HC.tanh_se(z, t)
    assert np.array_equal(a[0, [0, 2, 4]], [-1.0, 0.0, 1.0]) and np.allclose(dz, 2 * (a - t) * (1 - a * a), rtol=1e-15, atol=0)
    a, dz, loss = HC.identity_se(z, t)
    assert np.array_equal(a, z) and np.array_equal(dz, 2 * (z - t)) and loss[0] == ((z - t) ** 2).sum()
    # a numerical derivative of the loss, where nothing saturates
    for name in HC.HEADS:
        f = HC.HEADS[name]
        z0, y0 = np.array([0.3, -0.7, 1.1]), np.array([0.25, 0.5, 0.125])
        _, dz, _ = f(z0, y0)
        for i in range(3):
            e = np.zeros(3)
            e[i] = 1e-6
            num = (f(z0 + e, y0)[2] - f(z0 - e, y0)[2]) / 2e-6
            assert abs(num - dz[i]) < 1e-8, (name, i, num, dz[i])


def test_the_finite_cases_cover_every_width_of_the_table():
    for head, ws in HC.WIDTHS.items():
        for n in ws:
            for dt in HC.DTYPES:
                cases = HC.finite_cases(n, dt)
                assert {c["z"].shape for c in cases} == {(n,)} and {c["y"].shape for c in cases} == {(n,)}, (head, n)
                assert {c["pattern"] for c in cases} == set(HC.PATTERNS) and {c["target"] for c in cases} == set(HC.TARGETS)
                assert {c["nominal"] for c in cases} == set(HC.SPREADS)
    assert HC.WIDTHS["fused"] == (1, 2, 10, 16) and max(HC.WIDTHS["recon"]) == 1031 and max(HC.WIDTHS["wave"]) <= 64
