"""`induceNetwork` iterated in one call (to_fflayer_stack_induce; csrc/induce_seq.hip for the persistent route):
gradient descent on the input of an ffLayer stack with the parameters fixed (FeedForward.hs:150-164, app/MNIST.hs:357-365).

Checked against oracle.neuralnet.induceNetwork applied step by step on short runs, against the numpy restatement
(tests/induce_numpy.py) in fp64 on the application's run; then the routes (per iteration / persistent, forced on and off
and read back from to_induce_stats), determinism without a clock, and the call's contract.

No case skips because a result is off.  Stacks that fit one workgroup's LDS must run persistently when forced (asserted
from to_induce_stats).  A stack whose plan needs several workgroups a row may run per iteration under mode 2 where the
device does not place the workgroups of a group on one XCD: its results are checked all the same, and only the test that
compares persistent rows with each other skips then, with that reason."""
import ctypes as C
import functools
import gc
from contextlib import contextmanager

import numpy as np
import pytest

import induce_numpy as IN
from oracle import neuralnet as NN
from oracle.tensor import OTensor

pytestmark = pytest.mark.gpu
TOL = {np.float32: 1e-5, np.float64: 1e-12}
SOFTMAX, LOGISTIC, CROSS_ENTROPY, SQUARED_ERROR = 2, 0, 1, 0
HEADS = [("softmax", "crossEntropy"), ("logistic", "squaredError")]
SMALL = [[6, 4], [5, 9, 3], [7, 12, 8, 10], [3, 6, 5, 7, 40]]
APP = [784, 300, 100, 10]
O64 = OTensor(np.float64)


def ids(v):
    if isinstance(v, list):
        return "-".join(map(str, v))
    if isinstance(v, tuple):
        return v[0]
    return getattr(v, "__name__", str(v))


@pytest.fixture(scope="module")
def Ts():
    from tensor_ops_amd.hipt import HipT
    return {np.float32: HipT(0, np.float32), np.float64: HipT(0, np.float64)}


@contextmanager
def route(T, mode):
    T.induce_persistent(mode)
    try:
        yield
    finally:
        T.induce_persistent(1)


def one_workgroup(sizes, dt):
    """stacks the issue names as fitting ONE workgroup's LDS: they must run persistently when forced"""
    return sizes in ([2, 12, 8, 1], [7, 12, 8, 10], [6, 4], [5, 9, 3], [3, 6, 5, 7, 40]) or (sizes == [784, 32, 10] and dt == np.float32)


def put_net(T, ws):
    return [T.put(w) for w, _ in ws], [T.put(b) for _, b in ws]


def run(T, W, b, X, Y, rate, iters, head=HEADS[0], gx=False, losses=False, x_batched=True, y_batched=True):
    x = T.put(X, batched=x_batched)
    y = T.put(Y, batched=y_batched)
    out, g, ls = T.induce_stack(W, b, x, y, rate, iters, out_act=head[0], loss=head[1], want_gx=gx, want_losses=losses)
    return out.numpy(), (g.numpy() if g is not None else None), (ls.numpy() if ls is not None else None)


def ran(T, fn):
    """(result of fn, 'A' or 'B': the route to_induce_stats says ran -- exactly one call counted)"""
    p0, q0 = T.induce_stats()
    r = fn()
    p1, q1 = T.induce_stats()
    assert (p1 - p0) + (q1 - q0) == 1 and min(p1 - p0, q1 - q0) == 0, (p0, q0, p1, q1)
    return r, ("B" if p1 > p0 else "A")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


# ---- 1. oracle parity, short runs ---------------------------------------------------------------------------------------
def short_inputs(sizes, dt, soft):
    scale = 0.1 if sizes == [784, 32, 10] else 0.5
    rng = np.random.default_rng(len(sizes) * 100 + sizes[-1])
    ws = [((scale * rng.standard_normal((o, i))).astype(dt), (scale * rng.standard_normal(o)).astype(dt))
          for i, o in zip(sizes[:-1], sizes[1:])]
    X = rng.uniform(-1, 1, (16, sizes[0])).astype(dt)
    Y = np.zeros((16, sizes[-1]), dt)
    Y[np.arange(16), rng.integers(0, sizes[-1], 16)] = 1
    if soft:
        Y = rng.uniform(0.1, 1, (16, sizes[-1])).astype(dt)
    return ws, X, Y


@functools.lru_cache(maxsize=None)
def oracle_short(sizes, dtname, head, soft):
    """per row: x_1, x_2, x_8 of induceNetwork applied step by step in fp64, netGrad's input cotangent at x_0 and at x_7"""
    dt = np.dtype(dtname).type
    ws, X, Y = short_inputs(list(sizes), dt, soft)
    net = NN.genNet([(w.astype(np.float64), b.astype(np.float64)) for w, b in ws], NN.actLogistic,
                    NN.actSoftmax if head[0] == "softmax" else NN.actLogistic)
    ol = {"squaredError": NN.squaredError, "crossEntropy": NN.crossEntropy}[head[1]]()
    xs = {k: np.empty(X.shape) for k in (1, 2, 8)}
    gs = {k: np.empty(X.shape) for k in (1, 8)}
    for r in range(X.shape[0]):
        x, y = X[r].astype(np.float64), Y[r].astype(np.float64)
        for k in range(8):
            if k in (0, 7):
                gs[k + 1][r] = np.asarray(NN.netGrad(O64, ol, x, y, net)[0], np.float64)
            x = np.asarray(NN.induceNetwork(O64, ol, 0.3, y, net, x), np.float64)
            if k + 1 in xs:
                xs[k + 1][r] = x
    return xs, gs


@pytest.mark.parametrize("soft", [False, True], ids=["onehot", "soft"])
@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=ids)
@pytest.mark.parametrize("head", HEADS, ids=ids)
@pytest.mark.parametrize("sizes", SMALL + [[784, 32, 10]], ids=ids)
def test_parity_with_the_oracle(Ts, sizes, head, dt, soft):
    T = Ts[dt]
    ws, X, Y = short_inputs(sizes, dt, soft)
    xs, gs = oracle_short(tuple(sizes), np.dtype(dt).name, head, soft)
    W, b = put_net(T, ws)
    assert np.abs(xs[8] - X).max() >= 1e-2          # the steps move x by a thousand times the fp32 tolerance and more
    for iters in (1, 2, 8):
        got = {}
        for mode in (0, 2):
            with route(T, mode):
                (out, gx, _), r = ran(T, lambda: run(T, W, b, X, Y, 0.3, iters, head, gx=iters != 2))
            got[mode] = (out, gx)
            assert r == "A" if mode == 0 else (r == "B" or not one_workgroup(sizes, dt)), (mode, r)
            err = np.abs(out.astype(np.float64) - xs[iters]).max()
            print("induce parity", sizes, head[0], np.dtype(dt).name, "soft" if soft else "onehot", "iters", iters, "mode", mode,
                  "route", r, "err", err)
            assert err <= TOL[dt], (iters, mode, err)
            if gx is not None:
                gerr = np.abs(gx.astype(np.float64) - gs[iters]).max()
                assert gerr <= TOL[dt], (iters, mode, gerr)
        assert np.abs(got[0][0].astype(np.float64) - got[2][0]).max() <= TOL[dt]   # the routes agree
        if got[0][1] is not None:
            assert np.abs(got[0][1].astype(np.float64) - got[2][1]).max() <= TOL[dt]


# ---- 2. the application's run ---------------------------------------------------------------------------------------------
def app_inputs():
    rng = np.random.default_rng(7)
    ws = [(0.1 * rng.standard_normal((o, i)), 0.1 * rng.standard_normal(o)) for i, o in zip(APP[:-1], APP[1:])]
    X = rng.uniform(0, 0.05, (10, 784))
    return ws, X, np.eye(10)


@functools.lru_cache(maxsize=None)
def app_reference(dtname):
    """numpy in fp64 on the inputs as the device gets them (rounded to dt), and numpy carried in dt itself"""
    dt = np.dtype(dtname).type
    ws, X, Y = app_inputs()
    ws = [(w.astype(dt), b.astype(dt)) for w, b in ws]
    X, Y = X.astype(dt), Y.astype(dt)
    ref = IN.induce(ws, X, Y, 1.0, 300)
    own = IN.induce(ws, X, Y, 1.0, 300, dtype=dt)
    return ws, X, Y, ref, own


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=ids)
def test_the_applications_run_784_300_100_10(Ts, dt, mode):
    """`induceNum` of app/MNIST.hs on all ten digits, 300 steps at rate 1.  The fp32 bound: d = max |numpy fp32 - numpy fp64|
    of x_300 on the same inputs, allowed max(1e-5, 4 d) -- the factor pays for summation order and the fused epilogues' fast
    exponential, in which a device route differs from numpy's fp32 and numpy's two precisions do not differ from each
    other; d itself must stay <= 2.5e-6 so that a change of inputs cannot loosen the bound unnoticed."""
    T = Ts[dt]
    ws, X, Y, (x_ref, _, l_ref), (x_own, _, _) = app_reference(np.dtype(dt).name)
    tol = TOL[dt]
    if dt == np.float32:
        d = np.abs(x_own.astype(np.float64) - x_ref).max()
        print("induce app: d =", d)
        assert d <= 2.5e-6
        tol = max(1e-5, 4 * d)
    W, b = put_net(T, ws)
    with route(T, mode):
        (out, _, losses), r = ran(T, lambda: run(T, W, b, X, Y, 1.0, 300, losses=True))
    err = np.abs(out.astype(np.float64) - x_ref).max()
    lerr = (np.abs(losses.astype(np.float64) - l_ref) / np.maximum(1.0, l_ref)).max()
    print("induce app", np.dtype(dt).name, "mode", mode, "route", r, "err", err, "loss err", lerr)
    assert mode != 0 or r == "A"
    assert err <= tol, err
    assert losses.shape == (10, 300)
    assert lerr <= TOL[dt], lerr
    l0 = IN.grad_x(ws, X, Y, "softmax", "crossEntropy")[1]
    assert np.abs(losses[:, 0] - l0).max() <= TOL[dt] * max(1.0, l0.max())   # losses[:, 0] is the loss at x
    assert (losses[:, -1] < losses[:, 0]).all()


def test_the_routes_agree_on_the_applications_run(Ts):
    for dt in (np.float32, np.float64):
        T = Ts[dt]
        ws, X, Y, _, _ = app_reference(np.dtype(dt).name)
        W, b = put_net(T, ws)
        res = {}
        for mode in (0, 2):
            with route(T, mode):
                res[mode] = run(T, W, b, X, Y, 1.0, 300, losses=True)
        assert np.abs(res[0][0].astype(np.float64) - res[2][0]).max() <= TOL[dt]
        assert np.abs(res[0][2].astype(np.float64) - res[2][2]).max() <= TOL[dt] * max(1.0, res[0][2].max())


# ---- 3. the routes --------------------------------------------------------------------------------------------------------
def small_case(sizes, dt, B=8, seed=3, scale=0.5):
    rng = np.random.default_rng(seed)
    ws = [((scale * rng.standard_normal((o, i))).astype(dt), (scale * rng.standard_normal(o)).astype(dt))
          for i, o in zip(sizes[:-1], sizes[1:])]
    X = rng.uniform(-1, 1, (B, sizes[0])).astype(dt)
    Y = np.zeros((B, sizes[-1]), dt)
    Y[np.arange(B), rng.integers(0, sizes[-1], B)] = 1
    return ws, X, Y


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=ids)
def test_stats_count_the_route_that_ran(Ts, dt):
    T = Ts[dt]
    for sizes, head in (([2, 12, 8, 1], HEADS[1]), ([7, 12, 8, 10], HEADS[0])):
        ws, X, Y = small_case(sizes, dt)
        W, b = put_net(T, ws)
        for mode, want in ((0, "A"), (2, "B")):
            with route(T, mode):
                _, r = ran(T, lambda: run(T, W, b, X, Y, 0.3, 3, head))
            assert r == want, (sizes, mode)
    # no plan can hold this one: forced persistent, it runs per iteration and is right
    sizes = [64, 4096, 4096, 10]
    ws, X, Y = small_case(sizes, dt, B=4, scale=0.1)
    W, b = put_net(T, ws)
    with route(T, 2):
        (out, _, _), r = ran(T, lambda: run(T, W, b, X, Y, 0.3, 2))
    assert r == "A"
    want, _, _ = IN.induce(ws, X, Y, 0.3, 2)
    assert np.abs(want - X).max() > 0.05
    assert np.abs(out.astype(np.float64) - want).max() <= TOL[dt]


def test_launches_persistent_constant_per_iteration_growing(Ts):
    T = Ts[np.float32]
    ws, X, Y = small_case([7, 12, 8, 10], np.float32)
    W, b = put_net(T, ws)
    x, y = T.put(X, batched=True), T.put(Y, batched=True)

    def launches(iters):
        T.sync()
        l0 = T.stats()["launches"]
        T.induce_stack(W, b, x, y, 0.3, iters)
        return T.stats()["launches"] - l0
    with route(T, 2):
        launches(8)
        assert launches(8) == launches(128)
    with route(T, 0):
        l8, l128 = launches(8), launches(128)
    assert l128 >= l8 + 120


def test_the_setter(Ts):
    from tensor_ops_amd import capi
    T = Ts[np.float32]
    L = capi.lib()
    assert T.induce_persistent(1) == 1          # the default; tests restore it
    prev = C.c_int(-1)
    assert L.to_set_induce_persistent(3, C.byref(prev)) == 1 and L.to_set_induce_persistent(-1, None) == 1
    assert T.induce_persistent(0) == 1 and T.induce_persistent(2) == 0 and T.induce_persistent(1) == 2
    assert L.to_set_induce_persistent(1, None) == 0


# ---- 4. determinism, without a clock --------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 2])
@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=ids)
@pytest.mark.parametrize("sizes", [[7, 12, 8, 10], [784, 32, 10], [2, 12, 8, 1]], ids=ids)
def test_determinism(Ts, sizes, dt, mode):
    T = Ts[dt]
    head = HEADS[1] if sizes[-1] == 1 else HEADS[0]
    ws, X, Y = small_case(sizes, dt, B=9, scale=0.1 if sizes[0] > 100 else 0.5)
    W, b = put_net(T, ws)
    with route(T, mode):
        (a, ga, la), r = ran(T, lambda: run(T, W, b, X, Y, 0.3, 12, head, gx=True, losses=True))
        assert r == "A" if mode == 0 else (r == "B" or not one_workgroup(sizes, dt))
        a2, ga2, la2 = run(T, W, b, X, Y, 0.3, 12, head, gx=True, losses=True)
        assert np.array_equal(bits(a), bits(a2)) and np.array_equal(bits(ga), bits(ga2)) and np.array_equal(bits(la), bits(la2))
        # 5 then 7 on the result is 12
        m, _, lm = run(T, W, b, X, Y, 0.3, 5, head, losses=True)
        e, ge, le = run(T, W, b, m, Y, 0.3, 7, head, gx=True, losses=True)
        assert np.array_equal(bits(e), bits(a)) and np.array_equal(bits(ge), bits(ga))
        assert np.array_equal(bits(np.concatenate([lm, le], axis=1)), bits(la))
        # in place
        x, y = T.put(X, batched=True), T.put(Y, batched=True)
        o, _, _ = T.induce_stack(W, b, x, y, 0.3, 12, out_act=head[0], loss=head[1], in_place=True)
        assert o is x and np.array_equal(bits(x.numpy()), bits(a))
        # one unbatched target for every row is the tiled one
        Yt = np.tile(Y[0], (9, 1))
        t, gt, lt = run(T, W, b, X, Yt, 0.3, 12, head, gx=True, losses=True)
        u, gu, lu = run(T, W, b, X, Y[0], 0.3, 12, head, gx=True, losses=True, y_batched=False)
        assert np.array_equal(bits(t), bits(u)) and np.array_equal(bits(gt), bits(gu)) and np.array_equal(bits(lt), bits(lu))
        # an unbatched x is the one-row batch
        s, gs_, ls = run(T, W, b, X[0], Y[0], 0.3, 12, head, gx=True, losses=True, x_batched=False, y_batched=False)
        assert s.shape == (sizes[0],) and ls.shape == (12,)
        s1, g1, l1 = run(T, W, b, X[:1], Y[:1], 0.3, 12, head, gx=True, losses=True)
        assert np.array_equal(bits(s), bits(s1[0])) and np.array_equal(bits(gs_), bits(g1[0])) and np.array_equal(bits(ls), bits(l1[0]))


@pytest.mark.parametrize("case", [([7, 12, 8, 10], np.float32), ([7, 12, 8, 10], np.float64), ([784, 32, 10], np.float32),
                                  (APP, np.float32)], ids=lambda c: ids(c[0]) + "-" + c[1].__name__)
def test_persistent_row_does_not_depend_on_the_batch(Ts, case):
    sizes, dt = case
    T = Ts[dt]
    ws, X, Y = small_case(sizes, dt, B=37, scale=0.1 if sizes[0] > 100 else 0.5)
    W, b = put_net(T, ws)
    with route(T, 2):
        (full, gfull, lfull), r = ran(T, lambda: run(T, W, b, X, Y, 0.3, 6, gx=True, losses=True))
        if r == "A":
            assert not one_workgroup(sizes, dt)
            pytest.skip("the persistent plan of this stack needs several workgroups a row and the device does not place them on one XCD")
        for row in (0, 17, 36):
            (one, gone, lone), r1 = ran(T, lambda: run(T, W, b, X[row:row + 1], Y[row:row + 1], 0.3, 6, gx=True, losses=True))
            assert r1 == "B"
            assert np.array_equal(bits(one[0]), bits(full[row])) and np.array_equal(bits(gone[0]), bits(gfull[row]))
            assert np.array_equal(bits(lone[0]), bits(lfull[row]))


# ---- 5. contract ----------------------------------------------------------------------------------------------------------
def test_contract(Ts):
    from tensor_ops_amd import capi
    from tensor_ops_amd.hipt import Graph, _arr
    T, T64 = Ts[np.float32], Ts[np.float64]
    L = capi.lib()
    sizes = [7, 12, 8, 10]
    ws, X, Y = small_case(sizes, np.float32, B=20)
    W, b = put_net(T, ws)
    x, y = T.put(X, batched=True), T.put(Y, batched=True)
    for mode in (0, 2):
        with route(T, mode):
            # iters = 0: a bitwise copy, neither route counted
            s0 = T.induce_stats()
            out, _, _ = T.induce_stack(W, b, x, y, 0.3, 0)
            assert np.array_equal(bits(out.numpy()), bits(X)) and T.induce_stats() == s0
            xi = T.put(X, batched=True)
            T.induce_stack(W, b, xi, y, 0.3, 0, in_place=True)
            assert np.array_equal(bits(xi.numpy()), bits(X)) and T.induce_stats() == s0
            del out, xi
            # handles back where they were; parameters, x and y only read
            T.induce_stack(W, b, x, y, 0.3, 4, want_gx=True, want_losses=True)
            gc.collect()
            before = T.stats()
            res = T.induce_stack(W, b, x, y, 0.3, 4, want_gx=True, want_losses=True)
            del res
            gc.collect()
            after = T.stats()
            assert after["live_handles"] == before["live_handles"] and after["pool_bytes"] == before["pool_bytes"]
            for t, want in zip(W + b + [x, y], [w for w, _ in ws] + [bb for _, bb in ws] + [X, Y]):
                assert np.array_equal(bits(t.numpy()), bits(want))
            # a pending x inside a fusion scope is produced first
            want, _, _ = run(T, W, b, 2 * X, Y, 0.3, 4)
            with T.memo():
                x2 = T.scaleT(2.0, x)
                got, _, _ = T.induce_stack(W, b, x2, y, 0.3, 4)
                got = got.numpy()
            assert np.array_equal(bits(got), bits(want))

    sentinel = np.full((20, 7), 7.25, np.float32)
    out = T.put(sentinel, batched=True)

    def status(n=3, Wl=W, bl=b, hidden=LOGISTIC, out_act=SOFTMAX, loss=CROSS_ENTROPY, xx=x, yy=y, iters=2, oo=out, gg=None, ll=None):
        return L.to_fflayer_stack_induce(n, _arr(Wl), _arr(bl), hidden, out_act, loss, xx.h, yy.h, 0.3, iters, oo.h,
                                         gg.h if gg else None, ll.h if ll else None)

    def untouched():
        return np.array_equal(bits(out.numpy()), bits(sentinel))
    gxt = T.put(np.zeros((20, 7), np.float32), batched=True)
    checks = [
        (dict(iters=0, gg=gxt), 1),                                                         # gx of no iteration
        (dict(iters=-1), 1),
        (dict(n=0), 1),
        (dict(xx=T.put(X[:, :6], batched=True), oo=T.put(sentinel[:, :6], batched=True)), 2),   # x does not fit W_1
        (dict(Wl=[W[1], W[0], W[2]], bl=[b[1], b[0], b[2]]), 2),                            # layers do not chain
        (dict(yy=T.put(Y[:, :9], batched=True)), 2),                                        # y not n_L wide
        (dict(yy=T.put(Y[:19], batched=True)), 2),                                          # y of another batch
        (dict(xx=T.put(X[:19], batched=True)), 2),                                          # out of another batch
        (dict(gg=T.put(np.zeros((19, 7), np.float32), batched=True)), 2),
        (dict(ll=T.put(np.zeros((19, 2), np.float32), batched=True)), 2),                   # losses of another batch
        (dict(ll=T.put(np.zeros((20, 3), np.float32), batched=True)), 2),                   # losses not [B; iters]
        (dict(xx=T64.put(X.astype(np.float64), batched=True)), 1),                          # dtype mix
        (dict(out_act=SOFTMAX, loss=SQUARED_ERROR), 5),
        (dict(out_act=LOGISTIC, loss=CROSS_ENTROPY), 5),
        (dict(hidden=SOFTMAX), 5),
    ]
    for kw, want in checks:
        assert status(**kw) == want, kw
        assert untouched(), kw
    # a non-contiguous out: row 0 of a batched [2, 7] matrix
    wide = T.put(np.full((20, 2, 7), 7.25, np.float32), batched=True)
    view = T.slice(wide, (0,))
    assert status(oo=view) == 1
    assert np.array_equal(wide.numpy(), np.full((20, 2, 7), 7.25, np.float32))
    # refused while a capture records; the capture goes on
    T.scaleT(3.0, x)
    with Graph() as g:
        st = status()
        h = T.scaleT(3.0, x)
    assert st == 4 and untouched()
    g.launch()
    assert np.array_equal(h.numpy(), 3 * X)
    assert status() == 0 and not untouched()


# ---- 6. the large-batch end -----------------------------------------------------------------------------------------------
def test_large_batch_784_300_100_10(Ts):
    T = Ts[np.float32]
    ws, X, Y = small_case(APP, np.float32, B=4096, seed=11, scale=0.1)
    W, b = put_net(T, ws)
    assert T.induce_persistent(1) == 1
    (out, _, _), r = ran(T, lambda: run(T, W, b, X, Y, 0.3, 4))
    want, _, _ = IN.induce(ws, X, Y, 0.3, 4)
    err = np.abs(out.astype(np.float64) - want).max()
    print("induce large batch: route", r, "err", err)
    assert err <= 1e-5, err
