"""The case tables of tests/reduce_layout_cases.py, checked without a GPU: every case reaches the route it is annotated
with, every route of both restatements is reached in both element types, nothing needs more than 80 MB on the device, and
the references are the oracle's."""
import numpy as np
import pytest

import reduce_layout_cases as RC
from oracle import nested
from oracle.tensor import OTensor


@pytest.mark.parametrize("dt", RC.DTYPES, ids=["f32", "f64"])
def test_sum_cases_reach_their_routes_and_cover_all(dt):
    on, off = set(), set()
    extra = RC.sum_extra_off_cases(dt)   # (run with the switch off only)
    for c in RC.sum_cases(dt) + extra:
        O, R, J, sj = RC.sum_params(c)
        assert RC.sum_axis_route(O, R, J, sj, True) == c["route"], c["id"]
        assert RC.sum_axis_route(O, R, J, sj, False) == c["off_route"], c["id"]
        assert c in extra or RC.sum_case_bytes(c, dt, True) <= RC.MAX_DEVICE_BYTES, c["id"]
        assert RC.sum_case_bytes(c, dt, False) <= RC.MAX_DEVICE_BYTES, c["id"]
        on.add(c["route"])
        off.add(c["off_route"])
    assert RC.sum_axis_route(0, 5, 3, 1) == RC.sum_axis_route(4, 5, 0, 1) == "none"   # (no storage: nothing to run)
    assert on == set(RC.SUM_ROUTES) - {"none"}
    assert off == set(RC.SUM_ROUTES) - {"none", "column_sum"}
    # every route but the fill also on a NaN-surrounded view at an offset that is no multiple of 4
    views = [c for c in RC.SUM_CASES if c["view"]]
    assert {c["route"] for c in views} == set(RC.SUM_ROUTES) - {"none", "fill"}
    for c in views:
        assert int(np.prod(c["shape"])) % 4 != 0, c["id"]
    assert len({c["id"] for c in RC.SUM_CASES}) == len(RC.SUM_CASES)
    assert RC.sum_params(RC.grid_y_case(dt))[0] == 65537


def test_the_two_pass_cases_are_the_ones_described():
    assert RC.two_pass_split(256, 64) == (16, 16, 0, 16)
    assert RC.two_pass_split(4095, 64) == (255, 17, 14, 15)      # 14 empty trailing chunks, the last real one short
    assert RC.two_pass_split(1536, 4096)[0] == 4
    # the boundaries of the restatement itself
    assert RC.sum_axis_route(1, 4096, 64, 1) == "column_sum" and RC.sum_axis_route(1, 4095, 64, 1) == "two_pass"
    assert RC.sum_axis_route(1, 65536, 1, 0) == "partial" and RC.sum_axis_route(1, 65535, 1, 0) == "rows"
    assert RC.sum_axis_route(1, 255, 64, 1) == "cols" and RC.sum_axis_route(1, 256, 64, 1) == "two_pass"
    assert RC.sum_axis_route(64, 256, 1, 1) == "wave" and RC.sum_axis_route(64, 257, 1, 1) == "rows"
    assert RC.sum_axis_route(63, 10, 1, 1) == "rows"
    assert RC.sum_axis_route(1, 2048, 8192, 1, False) == "cols" and RC.sum_axis_route(1, 2048, 8128, 1, False) == "two_pass"


@pytest.mark.parametrize("dt", RC.DTYPES, ids=["f32", "f64"])
def test_copy_cases_reach_their_routes_and_cover_all(dt):
    seen = set()
    for c in RC.COPY_CASES:
        dims, st = RC.copy_case_view(c)
        assert RC.copy_route(dims, st) == c["route"], c["id"]
        assert 2 * (max(c["B"], 1) + 2) * int(np.prod(c["shape"])) * np.dtype(dt).itemsize <= RC.MAX_DEVICE_BYTES
        seen.add(c["route"])
    assert seen == set(RC.COPY_ROUTES)
    assert RC.copy_route([5, 4], [4, 1]) == "memcpy"                       # packed: merged into one run
    assert RC.copy_route([65536, 3, 2], [6, 1, 3]) == "general" and RC.copy_route([65535, 3, 2], [6, 1, 3]) == "transpose2d"
    assert RC.copy_route([65535 * 64 + 1, 2], [1, 65535 * 64 + 1]) == "general"
    assert RC.copy_route([0, 3], [3, 1]) == "none"


def test_the_other_tables_fit_the_device():
    for dt in RC.DTYPES:
        es = np.dtype(dt).itemsize
        for rank, n in RC.DIAG:
            assert 2 * n ** rank * es <= RC.MAX_DEVICE_BYTES
        assert 3 * 8195 * max(RC.gather_numels(dt)) * es <= RC.MAX_DEVICE_BYTES
        assert {n * es for n in RC.gather_numels(dt)} >= {8, 16, 3136}
    assert {n * 4 for n in RC.gather_numels(np.float32)} == {4, 8, 12, 16, 20, 3136}


def test_references_agree_with_the_oracle():
    rng = np.random.default_rng(5)
    O = OTensor(np.float64)
    x = rng.integers(-5, 6, (7, 3, 4)).astype(np.float64)
    case = {"entry": "sumRows", "shape": x.shape, "B": 0}
    assert np.array_equal(RC.sum_reference(case, x)[0], O.sumRows(x)) and np.array_equal(O.sumRows(x), nested.sum_rows(x))
    case = {"entry": "sumRows", "shape": x.shape[1:], "B": 7}
    assert np.array_equal(RC.sum_reference(case, x)[0], np.stack([O.sumRows(s) for s in x]))
    case = {"entry": "batch_sum", "shape": x.shape[1:], "B": 7}
    assert np.array_equal(RC.sum_reference(case, x)[0], O.sumT(list(x), x.shape[1:]))
    m = x[:3, :, :3].reshape(3, 9)[:, :3]
    assert RC.sum_reference({"entry": "trace", "shape": (3, 3), "B": 0}, m)[0] == O.getDiag(m).sum()
    for shape, B in (((2, 3, 5), 0), ((3, 1, 4), 0), ((2, 3), 4)):
        c = {"shape": shape, "B": B}
        y = np.arange(int(np.prod(shape)) * max(B, 1), dtype=np.float64).reshape(((B,) if B else ()) + shape)
        want = np.stack([O.transp(s) for s in y]) if B else O.transp(y)
        assert np.array_equal(RC.copy_reference(c, y), want)
        # the view `contiguous()` packs is that transpose
        dims, st = RC.copy_case_view(c)
        assert np.array_equal(np.lib.stride_tricks.as_strided(y, dims, [s * 8 for s in st]), want)


def test_arg_rows_hold_every_pattern_and_the_reference_is_the_fold():
    for n in RC.ARG_NS:
        for dt in RC.DTYPES:
            rows = RC.arg_rows(n, dt)
            assert rows.dtype == dt and rows.shape[1] == n
            nan = np.isnan(rows)
            assert nan.all(axis=1).any() and nan[:, 0].any() and nan[:, -1].any() and np.isinf(rows).any()
            if n >= 129:
                assert any(r[j] and r[j + 64] for r in nan for j in range(n - 64))   # two NaN on one lane
            finite = ~nan.any(axis=1)
            want = RC.arg_reference(rows)
            assert np.array_equal(want[finite], np.argmax(rows[finite], axis=1))     # earliest on ties, as numpy
            assert np.array_equal(RC.arg_reference(rows, True)[finite], np.argmin(rows[finite], axis=1))
    O = OTensor(np.float64)
    assert O.arg_max(np.array([1.0, np.nan, 0.5])) == 2 and O.arg_max(np.array([0.0, -0.0])) == 0
    assert O.arg_min(np.array([-0.0, 0.0])) == 0


def test_nan_fold_is_the_suffix_behind_the_last_nan():
    rows = RC.nan_property_rows()
    assert len(rows) == 1000 and {len(r) for r in rows} == {1, 2, 3, 63, 64, 65, 128, 129, 200}
    O = OTensor(np.float64)
    for r in rows:
        assert 1 <= np.isnan(r).sum() <= 3
        assert O.arg_max(r) == RC.arg_closed_form(r), r
        assert O.arg_min(r) == RC.arg_closed_form(r, True), r
