"""`online_sgd_kernel` (csrc/online_sgd.hip) and `induce_seq_kernel` (csrc/induce_seq.hip) at every edge of their plans and of
their unrolled loops: the cases, inputs, references and bounds of tests/persist_cases.py (checked against numpy alone by
tests/test_persist_cases.py).

Per case: the plan the case was written for is asserted against the library's own (`to_persist_plan_query`), the case runs, the
route (induce: `to_induce_stats`) or the one persistent launch (online: the launch counter) is asserted, the values are compared
with numpy in float64 elementwise, the updates row by row and column by column (online) or element by element (induce), X and Y
must come back bit for bit, and where several workgroups share the work a second run must give the same bits.

An online case skips only when the call fails with the library's own "do not share an XCD" message (the skip states it); nothing
skips because a value is off.  An induce case whose plan needs several workgroups a row runs per iteration on such a device, and
its values are checked all the same."""
import ctypes as C

import numpy as np
import pytest

import persist_cases as PC
from persist_cases import F32, F64

pytestmark = pytest.mark.gpu
NP = {F32: np.float32, F64: np.float64}
HIDDEN_ACT = {"logistic": 0, "tanh": 3}                    # TO_ACT_LOGISTIC, TO_ACT_TANH
HEAD = {"softmax": (2, 1, "softmax", "crossEntropy"), "logistic": (0, 0, "logistic", "squaredError")}
NO_XCD = b"do not share an XCD"


@pytest.fixture(scope="module")
def Ts():
    from tensor_ops_amd.hipt import HipT
    return {dt: HipT(0, NP[dt]) for dt in PC.DTYPES}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def assert_plan(q, stated, grid=None):
    if stated is None:
        assert not q["exists"] and (q["G"], q["slice"], q["last_slice"], q["lds_bytes"], q["grid"]) == (0, 0, 0, 0, 0), q
        return
    assert q["exists"] and (q["G"], q["slice"], q["last_slice"]) == tuple(stated), (q, stated)
    assert 0 < q["lds_bytes"] <= PC.LDS_MAX, q
    assert q["grid"] == (8 * q["G"] if grid is None else grid), q


# ---- online SGD -----------------------------------------------------------------------------------------------------------------
def run_online(T, dt, ws, X, Y, idx, n, rate, hidden, head):
    """(status, weights, biases, X, Y on the device, launches counted by the call)"""
    from tensor_ops_amd import capi
    dw = [T.put(w.astype(NP[dt])) for w, _ in ws]
    db = [T.put(b.astype(NP[dt])) for _, b in ws]
    wa = (capi.c_tensor * len(ws))(*[t.h for t in dw])
    ba = (capi.c_tensor * len(ws))(*[t.h for t in db])
    ia = (C.c_int64 * max(len(idx), 1))(*[int(v) for v in idx]) if idx is not None else None
    dX, dY = T.put(X.astype(NP[dt]), batched=True), T.put(Y.astype(NP[dt]), batched=True)
    T.sync()
    l0 = T.stats()["launches"]
    st = capi.lib().to_fflayer_stack_online_sgd(len(ws), wa, ba, HIDDEN_ACT[hidden], HEAD[head][0], HEAD[head][1], dX.h, dY.h, n, ia, rate)
    return st, dw, db, dX, dY, T.stats()["launches"] - l0


def skip_if_not_placed(st):
    from tensor_ops_amd import capi
    if st != 0 and NO_XCD in capi.lib().to_last_error():
        pytest.skip(capi.lib().to_last_error().decode())


def check_online_values(tag, dt, ws, want, dw, db):
    bound = PC.VALUE_BOUND["online"][dt]
    figures = []
    for l, ((w0, _), (ww, wb), gw, gb) in enumerate(zip(ws, want, dw, db)):
        gw, gb = gw.numpy(), gb.numpy()
        assert gw.dtype == NP[dt] and gb.dtype == NP[dt]
        ratio, where = PC.online_structure(gw, ww, w0)
        figures.append((PC.rel_max(gw, ww), PC.rel_max(gb, wb), ratio, where))
    print("persist edge online", tag, dt, " ".join("W%d %.2e b %.2e update %.2e@%d" % ((l + 1,) + f) for l, f in enumerate(figures)))
    for l, (ew, eb, ratio, where) in enumerate(figures):
        assert ew <= bound and eb <= bound, (tag, dt, "layer", l + 1, ew, eb)
        assert ratio <= PC.STRUCTURE, (tag, dt, "layer", l + 1, "row" if where < want[l][0].shape[0] else "column", where, ratio)


ONLINE_ACCEPTED = [(c, h, o, dt) for c in PC.ONLINE for dt in PC.DTYPES if c.plan[dt] is not None for h, o in PC.online_combos(c)]
ONLINE_REFUSED = [(c, dt) for c in PC.ONLINE for dt in PC.DTYPES if c.plan[dt] is None]


@pytest.mark.parametrize("case,hidden,head,dt", ONLINE_ACCEPTED, ids=lambda v: getattr(v, "id", v))
def test_online_case(Ts, case, hidden, head, dt):
    T, dims = Ts[dt], tuple(case.dims)
    q = T.persist_plan("online", dims)
    assert_plan(q, case.plan[dt])
    assert case.holds(case.dims, case.plan[dt], dt), case.why
    ws, X, Y, order = PC.online_inputs(dims, hidden, head)
    rate = PC.online_rate(dims, hidden, head)
    want = PC.online_reference(dims, hidden, head)
    st, dw, db, dX, dY, launches = run_online(T, dt, ws, X, Y, order, len(order), rate, hidden, head)
    skip_if_not_placed(st)
    assert st == 0 and q["placement_ok"]
    assert launches == 1                                                    # the one persistent launch
    check_online_values("%s %s %s" % (case.id, hidden, head), dt, ws, want, dw, db)
    assert np.array_equal(bits(dX.numpy()), bits(X.astype(NP[dt]))) and np.array_equal(bits(dY.numpy()), bits(Y.astype(NP[dt])))
    if q["G"] > 1:                                                          # workgroup-ordered sums: the same bits again
        st2, dw2, db2, _, _, _ = run_online(T, dt, ws, X, Y, order, len(order), rate, hidden, head)
        assert st2 == 0
        for a, b in zip(dw + db, dw2 + db2):
            assert np.array_equal(bits(a.numpy()), bits(b.numpy()))


@pytest.mark.parametrize("case,dt", ONLINE_REFUSED, ids=lambda v: getattr(v, "id", v))
def test_online_refuses(Ts, case, dt):
    """a stack outside the range: non-zero, the kernel named in to_last_error, every parameter bit-identical"""
    from tensor_ops_amd import capi
    T = Ts[dt]
    assert_plan(T.persist_plan("online", case.dims), None)
    rng = np.random.default_rng(5)
    ws = PC.draw_net(rng, case.dims, "logistic")
    X, Y = PC.draw_rows(rng, case.dims, 4, "softmax")
    st, dw, db, _, _, launches = run_online(T, dt, ws, X, Y, None, 4, 0.1, "logistic", "softmax")
    assert st != 0 and b"online SGD kernel" in capi.lib().to_last_error() and launches == 0
    for (w, b), gw, gb in zip(ws, dw, db):
        assert np.array_equal(bits(gw.numpy()), bits(w.astype(NP[dt]))) and np.array_equal(bits(gb.numpy()), bits(b.astype(NP[dt])))


@pytest.mark.parametrize("dt", PC.DTYPES)
def test_online_lds_limit_from_the_query(Ts, dt):
    """the largest o1 the plan accepts at the other widths of a pair, found by asking: the stated one fits 160 KiB, one row more
    does not, and ten rows less fits as well (the limit is no island)"""
    T = Ts[dt]
    for ok, refused in PC.ONLINE_LDS_LIMIT[dt]:
        a, b = PC.by_id(PC.ONLINE, ok), PC.by_id(PC.ONLINE, refused)
        qa, qb = T.persist_plan("online", a.dims), T.persist_plan("online", b.dims)
        print("persist edge lds limit", dt, a.id, qa["lds_bytes"], "of", PC.LDS_MAX)
        assert qa["exists"] and qa["lds_bytes"] <= PC.LDS_MAX and not qb["exists"]
        assert T.persist_plan("online", [a.dims[0], a.dims[1] - 10] + a.dims[2:])["exists"]
        if (a.id, dt) in PC.ONLINE_LDS_STATED:
            assert qa["lds_bytes"] == PC.ONLINE_LDS_STATED[(a.id, dt)]


@pytest.mark.parametrize("dt", PC.DTYPES)
@pytest.mark.parametrize("stream", PC.STREAM, ids=lambda s: s[0])
def test_online_stream_edges(Ts, stream, dt):
    sid, idx, n = stream
    T, dims = Ts[dt], tuple(PC.STREAM_DIMS)
    assert_plan(T.persist_plan("online", dims), PC.STREAM_PLAN)
    for hidden in PC.HIDDEN:
        for head in PC.HEADS:
            ws, X, Y, _ = PC.online_inputs(dims, hidden, head, PC.STREAM_ROWS)
            st, dw, db, dX, dY, launches = run_online(T, dt, ws, X, Y, idx, n, PC.online_rate(dims, hidden, head), hidden, head)
            skip_if_not_placed(st)
            assert st == 0
            if n == 0:
                assert launches == 0
                for (w, b), gw, gb in zip(ws, dw, db):
                    assert np.array_equal(bits(gw.numpy()), bits(w.astype(NP[dt]))) and np.array_equal(bits(gb.numpy()), bits(b.astype(NP[dt])))
                continue
            assert launches == 1
            order = tuple(idx) if idx is not None else tuple(range(n))
            want = PC.online_reference(dims, hidden, head, order=order, rows=PC.STREAM_ROWS)
            bound = PC.VALUE_BOUND["online"][dt]
            for (ww, wb), gw, gb in zip(want, dw, db):
                ew, eb = PC.rel_max(gw.numpy(), ww), PC.rel_max(gb.numpy(), wb)
                print("persist edge stream", sid, hidden, head, dt, "W %.2e b %.2e" % (ew, eb))
                assert ew <= bound and eb <= bound, (sid, hidden, head, ew, eb)
            assert np.array_equal(bits(dX.numpy()), bits(X.astype(NP[dt]))) and np.array_equal(bits(dY.numpy()), bits(Y.astype(NP[dt])))


# ---- induce ---------------------------------------------------------------------------------------------------------------------
def run_induce(T, dt, ws, X, Y, iters, hidden, head, y_batched=True):
    """under mode 2: ((x, gx, losses), the route that ran, x and y as they are on the device afterwards)"""
    W, b = [T.put(w.astype(NP[dt])) for w, _ in ws], [T.put(v.astype(NP[dt])) for _, v in ws]
    x, y = T.put(X.astype(NP[dt]), batched=True), T.put(Y.astype(NP[dt]), batched=y_batched)
    prev = T.induce_persistent(2)
    try:
        p0, q0 = T.induce_stats()
        out, gx, ls = T.induce_stack(W, b, x, y, PC.INDUCE_RATE, iters, out_act=HEAD[head][2], loss=HEAD[head][3], want_gx=True,
                                     want_losses=True, hidden_act=hidden)
        p1, q1 = T.induce_stats()
    finally:
        T.induce_persistent(prev)
    assert (p1 - p0) + (q1 - q0) == 1
    return (out.numpy(), gx.numpy(), ls.numpy()), ("B" if p1 > p0 else "A"), x.numpy(), y.numpy()


def check_induce(T, tag, case, dt, hidden, head, iters, rows=PC.INDUCE_ROWS, one_target=False):
    dims = tuple(case.dims)
    q = T.persist_plan("induce", dims, B=rows, iters=iters)
    stated = case.plan[dt]
    assert_plan(q, stated, grid=None if stated is None or stated[0] > 1 else min(rows, 256))
    assert case.holds(case.dims, stated, dt), case.why
    route = "B" if q["exists"] and (q["G"] == 1 or q["placement_ok"]) else "A"
    ws, X, Y = PC.induce_inputs(dims, hidden, head, rows)
    Yd = Y[0] if one_target else Y
    want = PC.induce_reference(dims, hidden, head, iters, rows=rows, one_target=one_target)
    own = PC.induce_reference(dims, hidden, head, iters, dtname=F32, rows=rows, one_target=one_target)
    mask = PC.induce_mask(want[0], own[0], X)
    got, r, x_after, y_after = run_induce(T, dt, ws, X, Yd, iters, hidden, head, y_batched=not one_target)
    errs = [PC.abs_max(g, w) for g, w in zip(got, want)]
    worst = PC.induce_structure(got[0], want[0], X, mask)
    print("persist edge induce", tag, dt, "iters", iters, "route", r, "x %.2e gx %.2e losses %.2e update %.2e" % (tuple(errs) + (worst,)))
    assert r == route, (r, q)
    assert got[0].dtype == NP[dt] and got[2].shape == (rows, iters)
    bound = PC.VALUE_BOUND["induce"][dt]
    assert max(errs) <= bound, (tag, dt, iters, errs)
    assert worst <= PC.STRUCTURE, (tag, dt, iters, worst)
    assert np.array_equal(bits(x_after), bits(X.astype(NP[dt]))) and np.array_equal(bits(y_after), bits(Yd.astype(NP[dt])))
    if q["exists"] and q["G"] > 1:
        again, r2, _, _ = run_induce(T, dt, ws, X, Yd, iters, hidden, head, y_batched=not one_target)
        assert r2 == r and all(np.array_equal(bits(a), bits(b)) for a, b in zip(got, again))


INDUCE_RUNS = [(c, h, o, dt) for c in PC.INDUCE for dt in PC.DTYPES if dt in c.plan for h in PC.HIDDEN for o in PC.HEADS]


@pytest.mark.parametrize("case,hidden,head,dt", INDUCE_RUNS, ids=lambda v: getattr(v, "id", v))
def test_induce_case(Ts, case, hidden, head, dt):
    for iters in PC.induce_iters(case, dt):
        check_induce(Ts[dt], "%s %s %s" % (case.id, hidden, head), case, dt, hidden, head, iters)


@pytest.mark.parametrize("dt", PC.DTYPES)
@pytest.mark.parametrize("rows", PC.INDUCE_ROW_COUNTS)
def test_induce_row_counts(Ts, rows, dt):
    """one row; and one row more than the grid's 256 workgroups: workgroup 0 takes rows 0 and 256"""
    case = PC.by_id(PC.INDUCE, PC.INDUCE_ROWS_CASE)
    for hidden in PC.HIDDEN:
        for head in PC.HEADS:
            check_induce(Ts[dt], "%s %s %s rows %d" % (case.id, hidden, head, rows), case, dt, hidden, head, PC.INDUCE_ITERS, rows=rows)


@pytest.mark.parametrize("dt", PC.DTYPES)
def test_induce_one_unbatched_target(Ts, dt):
    case = PC.by_id(PC.INDUCE, PC.INDUCE_ONE_TARGET_CASE)
    for hidden in PC.HIDDEN:
        for head in PC.HEADS:
            check_induce(Ts[dt], "%s %s %s one target" % (case.id, hidden, head), case, dt, hidden, head, PC.INDUCE_ITERS, one_target=True)


@pytest.mark.parametrize("dt", PC.DTYPES)
def test_induce_lds_stated(Ts, dt):
    for (cid, d), lds in PC.INDUCE_LDS_STATED.items():
        if d == dt:
            assert Ts[dt].persist_plan("induce", PC.by_id(PC.INDUCE, cid).dims, B=PC.INDUCE_ROWS, iters=1)["lds_bytes"] == lds


def test_query_refuses_bad_arguments(Ts):
    from tensor_ops_amd import capi
    L = capi.lib()
    d = (C.c_int64 * 8)(5, 4, 3)
    i = [C.c_int(-7) for _ in range(4)]
    lds, grid, ok = C.c_int64(-7), C.c_int64(-7), C.c_int(-7)
    outs = [C.byref(o) for o in i] + [C.byref(lds), C.byref(grid), C.byref(ok)]
    for args in ((2, 0, 2, d, 1, 1), (0, 7, 2, d, 1, 1), (0, 0, 0, d, 1, 1), (0, 0, 8, d, 1, 1), (0, 0, 2, None, 1, 1)):
        assert L.to_persist_plan_query(*args, *outs) != 0
        assert [o.value for o in i] + [lds.value, grid.value, ok.value] == [-7] * 7
    assert L.to_persist_plan_query(1, 0, 2, d, 0, 1, *outs) == 0 and i[0].value == 0      # B < 1: no plan, no error
