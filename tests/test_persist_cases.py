"""tests/persist_cases.py against the reference alone (no GPU): the ids are unique, every stated plan is a split of the width it
cuts, every case's branch property follows from its widths and its stated plan by the arithmetic restated there, and the
conditions under the bounds hold on every case's inputs --

  value      numpy carried in the element type stays within a quarter of the value bound of that type (float32 against float64;
             float64 against np.longdouble where that is wider, else unmeasured and said so);
  structure  online: on EVERY row and column of every weight matrix the update max|dwant| is at least 100 x numpy's float32
             drift there; induce: the same per element of x, at most 1 % of a row's elements under it.

Each test prints what it measured (`persist drift ...`); profiles/persist_edges_drift.txt is that output."""
import numpy as np
import pytest

import persist_cases as PC
from persist_cases import F32, F64

WIDER = np.finfo(np.longdouble).eps < 1e-18   # a yardstick for float64 exists on this machine


def test_ids_are_unique():
    for table in (PC.ONLINE, PC.INDUCE):
        ids = [c.id for c in table]
        assert len(set(ids)) == len(ids)
    assert len({s[0] for s in PC.STREAM}) == len(PC.STREAM)
    for pairs in PC.ONLINE_LDS_LIMIT.values():
        for pair in pairs:
            for cid in pair:
                PC.by_id(PC.ONLINE, cid)
    PC.by_id(PC.INDUCE, PC.INDUCE_ROWS_CASE)
    PC.by_id(PC.INDUCE, PC.INDUCE_ONE_TARGET_CASE)


@pytest.mark.parametrize("case", PC.ONLINE + PC.INDUCE, ids=lambda c: c.id)
def test_branch_follows_from_the_widths(case):
    width = case.dims[1] if case in PC.ONLINE else case.dims[0]     # online cuts o1 by rows, induce cuts i0 by columns
    assert set(case.plan) <= set(PC.DTYPES) and case.plan
    for dt, plan in case.plan.items():
        if plan is not None:
            assert PC.plan_is_a_split(width, plan), (case.id, dt, plan)
        assert case.holds(case.dims, plan, dt), (case.id, dt, case.why)


def test_lds_limit_pairs_differ_by_one_row():
    for dt, pairs in PC.ONLINE_LDS_LIMIT.items():
        for ok, refused in pairs:
            a, b = PC.by_id(PC.ONLINE, ok), PC.by_id(PC.ONLINE, refused)
            assert a.plan[dt] is not None and b.plan[dt] is None
            assert b.dims[1] == a.dims[1] + 1 and b.dims[:1] + b.dims[2:] == a.dims[:1] + a.dims[2:]
    for (cid, dt), lds in list(PC.ONLINE_LDS_STATED.items()) + list(PC.INDUCE_LDS_STATED.items()):
        assert lds <= PC.LDS_MAX


def test_stream_cases_are_valid():
    assert PC.plan_is_a_split(PC.STREAM_DIMS[1], PC.STREAM_PLAN)
    for sid, idx, n in PC.STREAM:
        assert (len(idx) == n and max(idx) < PC.STREAM_ROWS) if idx is not None else n <= PC.STREAM_ROWS


ONLINE_RUNS = [(c, h, o) for c in PC.ONLINE if any(p is not None for p in c.plan.values()) for h, o in PC.online_combos(c)]


@pytest.mark.parametrize("case,hidden,head", ONLINE_RUNS, ids=lambda v: getattr(v, "id", v))
def test_online_conditions(case, hidden, head):
    dims = tuple(case.dims)
    ws, X, Y, order = PC.online_inputs(dims, hidden, head)
    want = PC.online_reference(dims, hidden, head)
    own = PC.online_reference(dims, hidden, head, dtname=F32)
    drift = max(max(PC.rel_max(o[0], w[0]), PC.rel_max(o[1], w[1])) for o, w in zip(own, want))
    margin = min(PC.online_update_margin(w[0], o[0], i[0]) for w, o, i in zip(want, own, ws))
    d64 = None
    if WIDER:
        wide = PC.online_reference(dims, hidden, head, dtname="longdouble")
        d64 = max(max(float(np.abs(w[0] - x[0]).max() / np.abs(x[0]).max()), float(np.abs(w[1] - x[1]).max() / np.abs(x[1]).max()))
                  for w, x in zip(want, wide))
    print("persist drift online %-22s %-8s %-8s float32 %.2e  float64 %s  min update/drift %.0f"
          % (case.id, hidden, head, drift, "%.2e" % d64 if d64 is not None else "unmeasured", margin))
    assert drift <= PC.VALUE_BOUND["online"][F32] / 4
    assert d64 is None or d64 <= PC.VALUE_BOUND["online"][F64] / 4
    assert margin >= PC.MIN_UPDATE            # every row and every column: none left out


def test_stream_conditions():
    dims = tuple(PC.STREAM_DIMS)
    for hidden, head in [(h, o) for h in PC.HIDDEN for o in PC.HEADS]:
        for sid, idx, n in PC.STREAM:
            if n == 0:
                continue
            order = tuple(idx) if idx is not None else tuple(range(n))
            want = PC.online_reference(dims, hidden, head, order=order, rows=PC.STREAM_ROWS)
            own = PC.online_reference(dims, hidden, head, order=order, dtname=F32, rows=PC.STREAM_ROWS)
            drift = max(max(PC.rel_max(o[0], w[0]), PC.rel_max(o[1], w[1])) for o, w in zip(own, want))
            print("persist drift stream %-10s %-8s %-8s float32 %.2e" % (sid, hidden, head, drift))
            assert drift <= PC.VALUE_BOUND["online"][F32] / 4


INDUCE_RUNS = [(c, h, o) for c in PC.INDUCE for h in PC.HIDDEN for o in PC.HEADS]


@pytest.mark.parametrize("case,hidden,head", INDUCE_RUNS, ids=lambda v: getattr(v, "id", v))
def test_induce_conditions(case, hidden, head):
    dims = tuple(case.dims)
    ws, X, Y = PC.induce_inputs(dims, hidden, head)
    worst, worst64, left = 0.0, None, 0.0
    for iters in (1, 2, 3):
        want = PC.induce_reference(dims, hidden, head, iters)
        own = PC.induce_reference(dims, hidden, head, iters, dtname=F32)
        worst = max([worst] + [PC.abs_max(o, w) for o, w in zip(own, want)])
        mask = PC.induce_mask(want[0], own[0], X)
        left = max(left, (1 - mask.mean(axis=1)).max())
        if WIDER:
            wide = PC.induce_reference(dims, hidden, head, iters, dtname="longdouble")
            worst64 = max([worst64 or 0.0] + [float(np.abs(w - x).max()) for w, x in zip(want, wide)])
    print("persist drift induce %-22s %-8s %-8s float32 %.2e  float64 %s  left out %.2f %%"
          % (case.id, hidden, head, worst, "%.2e" % worst64 if worst64 is not None else "unmeasured", 100 * left))
    assert worst <= PC.VALUE_BOUND["induce"][F32] / 4
    assert worst64 is None or worst64 <= PC.VALUE_BOUND["induce"][F64] / 4
    assert left <= PC.INDUCE_LEFT_OUT


def test_induce_row_count_and_one_target_conditions():
    case = PC.by_id(PC.INDUCE, PC.INDUCE_ROWS_CASE)
    for rows in PC.INDUCE_ROW_COUNTS:
        for hidden, head in [(h, o) for h in PC.HIDDEN for o in PC.HEADS]:
            want = PC.induce_reference(tuple(case.dims), hidden, head, PC.INDUCE_ITERS, rows=rows)
            own = PC.induce_reference(tuple(case.dims), hidden, head, PC.INDUCE_ITERS, dtname=F32, rows=rows)
            X = PC.induce_inputs(tuple(case.dims), hidden, head, rows)[1]
            worst = max(PC.abs_max(o, w) for o, w in zip(own, want))
            left = (1 - PC.induce_mask(want[0], own[0], X).mean(axis=1)).max()
            print("persist drift induce %-22s %-8s %-8s rows %3d float32 %.2e  left out %.2f %%" % (case.id, hidden, head, rows, worst, 100 * left))
            assert worst <= PC.VALUE_BOUND["induce"][F32] / 4 and left <= PC.INDUCE_LEFT_OUT
    case = PC.by_id(PC.INDUCE, PC.INDUCE_ONE_TARGET_CASE)
    for hidden, head in [(h, o) for h in PC.HIDDEN for o in PC.HEADS]:
        want = PC.induce_reference(tuple(case.dims), hidden, head, PC.INDUCE_ITERS, one_target=True)
        own = PC.induce_reference(tuple(case.dims), hidden, head, PC.INDUCE_ITERS, dtname=F32, one_target=True)
        X = PC.induce_inputs(tuple(case.dims), hidden, head)[1]
        worst = max(PC.abs_max(o, w) for o, w in zip(own, want))
        left = (1 - PC.induce_mask(want[0], own[0], X).mean(axis=1)).max()
        print("persist drift induce %-22s %-8s %-8s one target float32 %.2e  left out %.2f %%" % (case.id, hidden, head, worst, 100 * left))
        assert worst <= PC.VALUE_BOUND["induce"][F32] / 4 and left <= PC.INDUCE_LEFT_OUT
