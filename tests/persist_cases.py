"""The cases of the two kernels whose workgroups share layer 1 through one XCD's L2 -- `online_sgd_kernel` (csrc/online_sgd.hip,
layer 1 split by ROWS) and `induce_seq_kernel` (csrc/induce_seq.hip, split by COLUMNS) -- at every edge of their plans and of
their hand-unrolled loops; with the inputs, the references and the bounds.  tests/test_persist_cases.py checks this file against
the reference alone (CPU); tests/test_gpu_persist_edges.py runs it.

A case names the branch it exists for (`why`), states the plan it was written for -- per element type (G, slice, last slice), or
None where the kernel must refuse the stack -- and carries `holds`: the branch property as arithmetic on the widths and the stated
plan, restated below from the kernels' loops.  The GPU test asserts the stated plan against the library (`to_persist_plan_query`),
so a change of a plan fails there instead of moving a case off its branch.

The references are act_numpy.online / act_numpy.induce; nothing here computes a network.

Inputs: W_l ~ N(0, (s / sqrt(fan_in))^2), b ~ 0.3 N(0, 1), X ~ U(-1, 1); one-hot targets for softmax, U(0.05, 0.95) for the
logistic head; s = 2 under logistic hidden layers, 1 under tanh.  Online: 16 samples out of 20 rows, in an order of their own;
rate 0.1 (logistic) or 0.05 (tanh).  Induce: 3 rows, up to 3 iterations, rate 0.3.  Everything is drawn in float32, so both element
types get the same numbers.  Larger rates or more samples make the float32 chain itself wander (numpy float32 against numpy
float64), which is what the conditions in test_persist_cases.py watch.

Bounds (elementwise; the figures of test_gpu_online.py / test_gpu_induce.py, which apply them by norm):
  online  per tensor   max|got - want| / max|want| <= 1e-5 (float32), 1e-11 (float64)
  induce               max|got - want|             <= 1e-5,           1e-12
  structure, online    every row and every column of every weight matrix: max|dgot - dwant| <= 0.1 max|dwant|, d = value - initial
  structure, induce    every element of x the same, but for the elements whose |dwant| is under 100 x numpy's float32 drift of
                       that element (at most 1 % of a row)
Conditions (CPU): numpy carried in the element type stays within a quarter of the value bound; every row's and column's
max|dwant| is at least 100 x numpy's float32 drift on it."""
import functools
from collections import namedtuple

import numpy as np

import act_numpy as AN

F32, F64 = "float32", "float64"
DTYPES = (F32, F64)
WORDS = {F32: 1, F64: 2}
VALUE_BOUND = {"online": {F32: 1e-5, F64: 1e-11}, "induce": {F32: 1e-5, F64: 1e-12}}
STRUCTURE = 0.1          # of the update, per row / column / element
MIN_UPDATE = 100.0       # x numpy's float32 drift: the condition under STRUCTURE
INDUCE_LEFT_OUT = 0.01   # of a row's elements
HIDDEN = ("logistic", "tanh")
HEADS = ("softmax", "logistic")
SCALE = {"logistic": 2.0, "tanh": 1.0}
ONLINE_RATE = {"logistic": 0.1, "tanh": 0.05}
ONLINE_SAMPLES, ONLINE_ROWS = 16, 20
INDUCE_RATE, INDUCE_ROWS, INDUCE_ITERS = 0.3, 3, 3
LDS_MAX = 160 * 1024
THREADS, NWV = 512, 8

Case = namedtuple("Case", "id dims plan why holds")


# ---- the kernels' loops, restated as counts ----------------------------------------------------------------------------------
def dot_passes(K, lane):
    """(unrolled passes, tail passes) of a lane in the four-chain dot product over K: `for (k = lane; k + 192 < K; k += 256)`,
    then `for (; k < K; k += 64)` (online layer 1, induce matvec's wave form)"""
    k, u, t = lane, 0, 0
    while k + 192 < K:
        k, u = k + 256, u + 1
    while k < K:
        k, t = k + 64, t + 1
    return u, t


def xregs(i0):
    """how many of the 512 threads hold an element in input register q = 0..3 (k = tid + 512 q < i0)"""
    return [max(0, min(THREADS, i0 - THREADS * q)) for q in range(4)]


def row_turns(nr):
    """turns of `for (r = wave; r < nr; r += 16)` taken by wave 0, and whether any wave pairs rows r, r + 8"""
    return -(-nr // (2 * NWV)), nr > NWV


def turns(n):
    """turns of `for (j = tid; j < n; j += 512)` taken by thread 0"""
    return -(-n // THREADS)


def online_exchange(G, o2, dt):
    """(32-bit words, polling passes of 2048 words, words of the last pass)"""
    total = G * o2 * WORDS[dt]
    return total, -(-total // (4 * THREADS)), total - (-(-total // (4 * THREADS)) - 1) * 4 * THREADS


def matvec_form(K):
    return "wave" if K >= 64 else "thread"


def matvec_t_runs(O, K):
    """(runs, rows a run, empty runs) of matvec_t; one run: the wide form, a thread a column over all rows"""
    nch = min(THREADS // K if K <= THREADS else 1, 16, O)
    if nch <= 1:
        return 1, O, 0
    ln = -(-O // nch)
    return nch, ln, sum(1 for q in range(nch) if q * ln >= O)


def plan_is_a_split(width, plan):
    """G slices of `slice` cover `width`, the last one `last` wide and not empty"""
    G, sl, last = plan
    return 1 <= G <= 32 and -(-width // sl) == G and last == width - (G - 1) * sl and 1 <= last <= sl


def both(p):
    return {F32: p, F64: p}


# ---- online SGD ---------------------------------------------------------------------------------------------------------------
ONLINE = [
    # tails of the four chains a lane and of the four input registers a thread
    Case("on-64-1-1", [64, 1, 1], both((1, 1, 1)), "o1 = oL = 1: one tail pass, no unrolled pass",
         lambda d, p, dt: dot_passes(d[0], 0) == (0, 1) and dot_passes(d[0], 63) == (0, 1)),
    Case("on-193-9-64", [193, 9, 64], both((9, 1, 1)), "unrolled pass entered by lane 0 only; oL = 64: a full wave in the head; L = 2",
         lambda d, p, dt: dot_passes(d[0], 0) == (1, 0) and dot_passes(d[0], 1) == (0, 3) and d[-1] == 64 and len(d) == 3),
    Case("on-257-5-3", [257, 5, 3], both((5, 1, 1)), "one unrolled pass, then a tail for lane 0; z2: one group of four plus one",
         lambda d, p, dt: dot_passes(d[0], 0) == (1, 1) and dot_passes(d[0], 1) == (1, 0) and divmod(p[0], 4) == (1, 1)),
    Case("on-513-35-10", [513, 35, 10], both((18, 2, 1)), "second input register holds one element; ragged last slice",
         lambda d, p, dt: xregs(d[0]) == [512, 1, 0, 0] and p[2] < p[1]),
    Case("on-1537-3-2", [1537, 3, 2], both((3, 1, 1)), "fourth input register holds one element",
         lambda d, p, dt: xregs(d[0]) == [512, 512, 512, 1]),
    Case("on-2048-40-7", [2048, 40, 7], both((20, 2, 2)), "all four input registers full: the widest input",
         lambda d, p, dt: xregs(d[0]) == [512] * 4),
    Case("on-2049-40-7", [2049, 40, 7], both(None), "one element beyond the input registers: refused",
         lambda d, p, dt: d[0] == 4 * THREADS + 1),
    # rows a workgroup
    Case("on-5-530-3", [5, 530, 3], both((32, 17, 3)), "rpw 17: a wave takes a third row (r and r + 8 together, then r + 16 alone); last workgroup single rows only",
         lambda d, p, dt: row_turns(p[1]) == (2, True) and p[1] > 16 and row_turns(p[2]) == (1, False)),
    Case("on-5-544-4", [5, 544, 4], both((32, 17, 17)), "rpw 17 in every workgroup",
         lambda d, p, dt: p[1] == p[2] == 17 and row_turns(17)[0] == 2),
    # widths past the workgroup
    Case("on-3-2-600-5", [3, 2, 600, 5], both((2, 1, 1)), "o2 = 600: second turn of every j loop and of the replicated layer's backward k loop; float64: two polling passes",
         lambda d, p, dt: turns(d[2]) == 2 and online_exchange(p[0], d[2], dt)[1] == WORDS[dt]),
    Case("on-6-33-520-3", [6, 33, 520, 3], both((17, 2, 1)), "8840 exchange words: five passes, the last partial; z2: four groups of four plus one",
         lambda d, p, dt: (dt != F32 or online_exchange(p[0], d[2], dt) == (8840, 5, 648)) and divmod(p[0], 4) == (4, 1) and turns(d[2]) == 2),
    # depth
    Case("on-65-66-130-9-3", [65, 66, 130, 9, 3], both((22, 3, 3)), "K = 130: ragged lane loop in a replicated layer; O = 9: more outputs than waves",
         lambda d, p, dt: d[2] % 64 != 0 and d[2] > 128 and d[3] > NWV),
    Case("on-9-7-6-5-4-3-2", [9, 7, 6, 5, 4, 3, 2], both((7, 1, 1)), "L = 6: the deepest stack",
         lambda d, p, dt: len(d) - 1 == 6),
    Case("on-9-7-6-5-4-3-2-2", [9, 7, 6, 5, 4, 3, 2, 2], both(None), "L = 7: refused",
         lambda d, p, dt: len(d) - 1 == 7),
    # the LDS limit: the largest o1 at these other widths and its successor, per element type (the GPU test re-derives each pair
    # from the query: accepted within 160 KiB, the next one refused)
    Case("on-1000-1120-64", [1000, 1120, 64], {F32: (32, 35, 35), F64: None}, "float32: the largest o1 at i0 = 1000, o2 = 64 (162 628 bytes)",
         lambda d, p, dt: dt != F32 or p[1] == 35),
    Case("on-1000-1121-64", [1000, 1121, 64], both(None), "float32: first refused", lambda d, p, dt: True),
    Case("on-784-1280-100-10", [784, 1280, 100, 10], {F32: (32, 40, 40), F64: None}, "float32: the largest o1 of the application's stack (163 288 bytes); the heaviest case",
         lambda d, p, dt: dt != F32 or p[1] == 40),
    Case("on-784-1281-100-10", [784, 1281, 100, 10], both(None), "float32: first refused", lambda d, p, dt: True),
    Case("on-1000-512-64", [1000, 512, 64], both((32, 16, 16)), "float64: the largest o1 at i0 = 1000, o2 = 64; rpw 16: two full turns of paired rows",
         lambda d, p, dt: row_turns(p[1]) == (1, True) and p[1] == 16),
    Case("on-1000-513-64", [1000, 513, 64], {F32: (31, 17, 3), F64: None}, "float64: first refused (float32: 31 workgroups)",
         lambda d, p, dt: True),
    Case("on-784-544-100-10", [784, 544, 100, 10], both((32, 17, 17)), "float64: the largest o1 of the application's stack",
         lambda d, p, dt: p[1] == 17),
    Case("on-784-545-100-10", [784, 545, 100, 10], {F32: (31, 18, 5), F64: None}, "float64: first refused (float32: 31 workgroups)",
         lambda d, p, dt: True),
]
# (largest accepted, first refused) per element type
ONLINE_LDS_LIMIT = {F32: [("on-1000-1120-64", "on-1000-1121-64"), ("on-784-1280-100-10", "on-784-1281-100-10")],
                    F64: [("on-1000-512-64", "on-1000-513-64"), ("on-784-544-100-10", "on-784-545-100-10")]}
ONLINE_LDS_STATED = {("on-1000-1120-64", F32): 162628, ("on-784-1280-100-10", F32): 163288}

# stream edges, on one small stack: (id, idx or None, n_idx)
STREAM_DIMS, STREAM_PLAN = [12, 5, 9, 4], (5, 1, 1)
STREAM = [
    ("n0", None, 0),                    # nothing to do: status 0, parameters bit-identical
    ("n1", [3], 1),                     # the two-deep prefetch of row index and row
    ("n2", [3, 0], 2),
    ("n3", [3, 0, 7], 3),
    ("repeat", [2, 2, 2, 0], 4),        # one row three times running
    ("null-idx", None, 5),              # rows 0..4 of a batch of 8
]
STREAM_ROWS = 8


def online_combos(case):
    """(hidden, head) pairs of a case: softmax with one output has no gradient (p = 1 = y), so it is left to the logistic head"""
    return [(h, o) for h in HIDDEN for o in HEADS if not (o == "softmax" and case.dims[-1] == 1)]


def _seed(*parts):
    """a seed that depends on the case alone (not on the process: `hash` of a string does)"""
    return sum((i + 1) * ord(c) for i, c in enumerate("/".join(map(str, parts))))


def draw_net(rng, dims, hidden):
    s = SCALE[hidden]
    return [((s / np.sqrt(i) * rng.standard_normal((o, i))).astype(np.float32), (0.3 * rng.standard_normal(o)).astype(np.float32))
            for i, o in zip(dims[:-1], dims[1:])]


def draw_rows(rng, dims, rows, head):
    X = rng.uniform(-1, 1, (rows, dims[0])).astype(np.float32)
    if head == "softmax":
        Y = np.zeros((rows, dims[-1]), np.float32)
        Y[np.arange(rows), rng.integers(0, dims[-1], rows)] = 1
    else:
        Y = rng.uniform(0.05, 0.95, (rows, dims[-1])).astype(np.float32)
    return X, Y


# Which draw of its inputs a run takes (0 unless named here), and a smaller rate where the listed one is too large.  Both were
# chosen on the CPU, from numpy alone: the first draw, then the first halving of the rate, at which the conditions of
# test_persist_cases.py hold.  What the draws before them measured (profiles/persist_edges_drift.txt has the rest):
DRAW = {
    ("online", (64, 1, 1), "tanh", "logistic"): 1,                # draw 0: a column of W1 (ONE element) moves 49 x its drift
    ("online", (3, 2, 600, 5), "logistic", "logistic"): 3,        # draws 0..2: a row of W2 (two elements) moves 51, 54, 31 x
    ("online", (3, 2, 600, 5), "tanh", "softmax"): 1,             # draw 0: float32 drift 3.2e-6, over a quarter of the bound
    ("online", (3, 2, 600, 5), "tanh", "logistic"): 4,            # draws 0..3: 21, 80, 65, 68 x
    ("online", (9, 7, 6, 5, 4, 3, 2), "logistic", "logistic"): 2,  # draw 0: 55 x; draw 1: 107 x, too close to tell
    # 257 rows of 63 elements: 1 % of a row is no element at all, and about one element in 16 000 moves under 100 x its drift
    ("induce", (63, 5, 3), "logistic", "logistic", 257): 1,
    ("induce", (63, 5, 3), "tanh", "softmax", 257): 1,
    ("induce", (63, 5, 3), "tanh", "logistic", 257): 10,          # draws 0..8 leave out 1 to 4 elements, draw 9 holds at 105 x
}
# 1120 logistic units into a logistic head at rate 0.1: a sample moves z2 by about rate |h1|^2 = 35 times dz2, the chain
# oscillates and float32 wanders 1e-4 .. 1e-3 from float64 on every draw tried; at half the rate 7e-7
RATE_SCALE = {("online", (1000, 1120, 64), "logistic", "logistic"): 0.5}


def online_rate(dims, hidden, head):
    return ONLINE_RATE[hidden] * RATE_SCALE.get(("online", tuple(dims), hidden, head), 1.0)


@functools.lru_cache(maxsize=None)
def online_inputs(dims, hidden, head, rows=ONLINE_ROWS, samples=ONLINE_SAMPLES):
    """(ws, X, Y, order) in float32; the caller must not write into them"""
    rng = np.random.default_rng(_seed("online", dims, hidden, head) + DRAW.get(("online", dims, hidden, head), 0))
    ws = draw_net(rng, dims, hidden)
    X, Y = draw_rows(rng, dims, rows, head)
    order = rng.permutation(rows)[:samples]
    return ws, X, Y, order


@functools.lru_cache(maxsize=None)
def online_reference(dims, hidden, head, order=None, dtname=F64, rows=ONLINE_ROWS):
    """the parameters after the stream, by act_numpy.online carried in `dtname`; order None: the case's own"""
    ws, X, Y, own = online_inputs(dims, hidden, head, rows)
    dt = np.dtype(dtname).type
    return AN.online(ws, X.astype(dt), Y.astype(dt), own if order is None else order, online_rate(dims, hidden, head), hidden, head, dt)


@functools.lru_cache(maxsize=None)
def induce_inputs(dims, hidden, head, rows=INDUCE_ROWS):
    rng = np.random.default_rng(_seed("induce", dims, hidden, head) + DRAW.get(("induce", dims, hidden, head, rows), 0))
    ws = draw_net(rng, dims, hidden)
    X, Y = draw_rows(rng, dims, rows, head)
    return ws, X, Y


@functools.lru_cache(maxsize=None)
def induce_reference(dims, hidden, head, iters, dtname=F64, rows=INDUCE_ROWS, one_target=False):
    """(x_iters, gx, losses) by act_numpy.induce carried in `dtname`; one_target: row 0's target for every row"""
    ws, X, Y = induce_inputs(dims, hidden, head, rows)
    dt = np.dtype(dtname).type
    return AN.induce(ws, X.astype(dt), (Y[0] if one_target else Y).astype(dt), INDUCE_RATE, iters, hidden, head, dt)


# ---- the measures ---------------------------------------------------------------------------------------------------------------
def f64(a):
    return np.asarray(a, np.float64)


def rel_max(got, want):
    """max|got - want| / max|want|"""
    return np.abs(f64(got) - f64(want)).max() / max(np.abs(f64(want)).max(), 1e-300)


def abs_max(got, want):
    return np.abs(f64(got) - f64(want)).max()


def rows_and_columns(a):
    """max|a| over every row, then over every column"""
    a = np.abs(f64(a))
    return np.concatenate([a.max(axis=1), a.max(axis=0)])


def online_structure(got, want, init):
    """(worst ratio max|dgot - dwant| / max|dwant| over the rows and columns of one weight matrix, its index: rows first)"""
    err = rows_and_columns(f64(got) - f64(want))
    upd = rows_and_columns(f64(want) - f64(init))
    ratio = err / np.maximum(upd, 1e-300)
    return ratio.max(), int(ratio.argmax())


def online_update_margin(want, own, init):
    """the condition: min over rows and columns of max|dwant| / numpy's drift in the element type on the same row or column"""
    upd = rows_and_columns(f64(want) - f64(init))
    drift = rows_and_columns(f64(own) - f64(want))
    return (upd / np.maximum(drift, 1e-300)).min()


def induce_mask(want, own, x0):
    """elements of x the structure bound is applied to: |dwant| >= 100 x numpy's float32 drift of that element"""
    return np.abs(f64(want) - f64(x0)) >= MIN_UPDATE * np.abs(f64(own) - f64(want))


def induce_structure(got, want, x0, mask):
    d = np.abs(f64(got) - f64(want))[mask] / np.abs(f64(want) - f64(x0))[mask]
    return d.max() if d.size else 0.0


# ---- induce ---------------------------------------------------------------------------------------------------------------------
def _i(dims, plan, why, holds):
    return Case("in-" + "-".join(map(str, dims)), dims, plan, why, holds)


INDUCE = [
    # matvec: a thread a row against a wave a row
    _i([63, 5, 3], both((1, 63, 63)), "layer 1 by a thread a row (K = 63)", lambda d, p, dt: matvec_form(p[1]) == "thread"),
    _i([64, 5, 3], both((1, 64, 64)), "layer 1 by a wave a row, one tail pass a lane (K = 64)",
       lambda d, p, dt: matvec_form(p[1]) == "wave" and dot_passes(64, 0) == (0, 1)),
    _i([65, 5, 3], both((1, 65, 65)), "wave a row, a second tail pass for lane 0 only",
       lambda d, p, dt: dot_passes(65, 0) == (0, 2) and dot_passes(65, 1) == (0, 1)),
    _i([257, 9, 3], both((1, 257, 257)), "matvec: unrolled pass plus tail; matvec_t of layer 1: one run, the wide form",
       lambda d, p, dt: dot_passes(257, 0) == (1, 1) and matvec_t_runs(d[1], p[1])[0] == 1),
    # matvec_t
    _i([256, 9, 3], both((1, 256, 256)), "matvec_t of layer 1: two runs", lambda d, p, dt: matvec_t_runs(d[1], p[1]) == (2, 5, 0)),
    _i([20, 33, 9, 4], both((1, 20, 20)), "matvec_t of layer 1: 16 runs of 3 rows over 33 rows, runs 11..15 empty; layer 2: 9 runs of one row",
       lambda d, p, dt: matvec_t_runs(d[1], p[1]) == (16, 3, 5) and matvec_t_runs(d[2], d[1]) == (9, 1, 0)),
    # wider than the workgroup
    _i([8, 600, 5], both((1, 8, 8)), "a thread a row with 600 rows; replicated K = 600: matvec_t wide with two turns, matvec two unrolled passes plus tail",
       lambda d, p, dt: matvec_form(p[1]) == "thread" and turns(d[1]) == 2 and matvec_t_runs(d[2], d[1])[0] == 1
       and dot_passes(600, 0) == (2, 2) and dot_passes(600, 63) == (2, 1)),
    _i([20, 513, 6, 4], both((1, 20, 20)), "replicated K = 513: one column past the workgroup",
       lambda d, p, dt: matvec_t_runs(d[2], d[1])[0] == 1 and turns(d[1]) == 2),
    # several workgroups a row
    _i([1300, 40, 3], {F32: (2, 650, 650), F64: (3, 434, 432)}, "float32: a slice wider than the workgroup; float64: three workgroups, ragged",
       lambda d, p, dt: turns(p[1]) == 2 if dt == F32 else p[2] < p[1]),
    _i([1561, 200, 3], {F32: (9, 174, 169)}, "G = 9: polling groups 8 + 1", lambda d, p, dt: divmod(p[0], 8) == (1, 1)),
    _i([745, 200, 3], {F64: (9, 83, 81)}, "G = 9 in float64: polling groups 8 + 1, 16 words in flight", lambda d, p, dt: divmod(p[0], 8) == (1, 1)),
    _i([977, 600, 3], {F32: (17, 58, 49)}, "G = 17: polling groups 8 + 8 + 1; o1 = 600: two exchange turns a thread; last slice a thread a row",
       lambda d, p, dt: divmod(p[0], 8) == (2, 1) and turns(d[1]) == 2 and matvec_form(p[2]) == "thread"),
    _i([1489, 200, 3], {F64: (17, 88, 81)}, "G = 17 in float64", lambda d, p, dt: divmod(p[0], 8) == (2, 1)),
    _i([1892, 600, 3], {F32: (32, 60, 32)}, "G = 32, a last slice half as wide", lambda d, p, dt: p[0] == 32 and p[2] < p[1]),
    _i([838, 600, 3], {F64: (32, 27, 1)}, "G = 32 in float64, the last slice ONE column", lambda d, p, dt: p[0] == 32 and p[2] == 1),
    _i([800, 300, 100, 10], {F32: (32, 25, 25)}, "the largest i0 at the application's widths (161 580 bytes)", lambda d, p, dt: p[0] == 32),
    _i([801, 300, 100, 10], {F32: None}, "no plan: per iteration", lambda d, p, dt: True),
]
INDUCE_LDS_STATED = {("in-800-300-100-10", F32): 161580}
# rows: on in-63-5-3, one row, and one row more than the grid's 256 workgroups (workgroup 0 takes rows 0 and 256)
INDUCE_ROW_COUNTS = (1, 257)
INDUCE_ROWS_CASE = "in-63-5-3"
INDUCE_ONE_TARGET_CASE = "in-1300-40-3"     # y unbatched (y_sm = 0), several workgroups a row


def induce_iters(case, dt):
    """every G > 1 case runs 1, 2 and 3 iterations: with 3, the second row starts on the odd exchange buffer with a running tag"""
    p = case.plan[dt]
    return (1, 2, 3) if p is not None and p[0] > 1 else (INDUCE_ITERS,)


def by_id(cases, cid):
    return next(c for c in cases if c.id == cid)
