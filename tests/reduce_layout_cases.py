"""Case tables, routing restatements and references for the kernels of csrc/reduce_layout.hip (test infrastructure; imports
no GPU code).  tests/test_reduce_layout_cases.py checks the tables on the CPU, tests/test_gpu_reduce_layout.py runs them.

`sum_axis_route` restates the predicates of `sum_axis_t`, `copy_route` the squeeze / merge / dispatch of `copy_strided_t`:
every table case carries the route it is meant to reach, the CPU test checks the annotation against the restatement, and
the GPU test checks the restatement against the library through the launch counter."""
import itertools

import numpy as np

from oracle.tensor import OTensor

SUM_ROUTES = ("none", "fill", "column_sum", "partial", "two_pass", "cols", "wave", "rows")
COPY_ROUTES = ("memcpy", "transpose2d", "general")
# launches of one launch_sum_axis call, per route (column_sum: gemv.hip splits the reduction or not)
SUM_LAUNCHES = {"none": (0,), "fill": (1,), "column_sum": (1, 2), "partial": (2,), "two_pass": (2,), "cols": (1,),
                "wave": (1,), "rows": (1,)}
MAX_DEVICE_BYTES = 80 * 1000 * 1000
DTYPES = (np.float32, np.float64)


def sum_axis_route(O, R, J, sj, gemv_on=True):
    """out[o, j] = sum_i x[o so + i si + j sj]: which kernel(s) `sum_axis_t` launches"""
    OJ = O * J
    if OJ == 0:
        return "none"
    if R == 0:
        return "fill"
    if O == 1 and sj == 1 and gemv_on and R * J >= (1 << 18):
        return "column_sum"
    if OJ == 1 and R >= (1 << 16):
        return "partial"
    nbx = (J + 63) // 64
    if O == 1 and J >= 64 and sj == 1 and R >= 256 and nbx < 128:
        rs = min(256 // nbx, R // 16)
        if rs >= 2:
            return "two_pass"
    if J >= 64 and sj == 1:
        return "cols"
    if R <= 256 and OJ >= 64:
        return "wave"
    return "rows"


def two_pass_split(R, J):
    """(rs, chunk, empty trailing chunks, rows of the last real chunk) of the two-pass column route"""
    nbx = (J + 63) // 64
    rs = min(256 // nbx, R // 16)
    chunk = (R + rs - 1) // rs
    real = (R + chunk - 1) // chunk
    return rs, chunk, rs - real, R - (real - 1) * chunk


def copy_route(dims, strides):
    """packing a strided view (dims with the batch, if any, leading): what `copy_strided_t` does with it"""
    total = int(np.prod(dims)) if len(dims) else 1
    if total == 0:
        return "none"
    d, st = [], []
    for n, s in zip(dims, strides):
        if n == 1:
            continue
        if d and st[-1] == s * n:
            d[-1] *= n
            st[-1] = s
        else:
            d.append(n)
            st.append(s)
    if not d:
        d, st = [1], [1]
    if len(d) == 1 and st[0] == 1:
        return "memcpy"
    if (len(d) == 2 and st[0] == 1) or (len(d) == 3 and st[1] == 1):
        o = 1 if len(d) == 3 else 0
        nb = d[0] if len(d) == 3 else 1
        if nb <= 65535 and (d[o] + 63) // 64 <= 65535:
            return "transpose2d"
    return "general"


def packed_strides(shape):
    st, p = [], 1
    for n in reversed(shape):
        st.append(p)
        p *= n
    return list(reversed(st))


def transp_view(shape, batch=0):
    """(dims, strides) of `transp` of a packed tensor, the batch leading, as `contiguous()` hands them to the copy"""
    dims, st = list(reversed(shape)), list(reversed(packed_strides(shape)))
    if batch > 0:
        dims, st = [batch] + dims, [int(np.prod(shape))] + st
    return dims, st


# ---- (a) sums ------------------------------------------------------------------------------------------------------------
# entry: sumRows (B = 0: unbatched, O = 1; else O = B), batch_sum (R = B, J = numel), blas_sum (sj = 0), trace (si = n + 1)
# view: the operand is a batch_select / batch_slice view of the interior of a NaN-filled tensor, at an element offset that is
#       no multiple of 4 (the case's numel is chosen for that)
def _s(entry, shape, route, B=0, view=False, off_route=None):
    return {"entry": entry, "shape": tuple(shape), "B": B, "route": route, "view": view,
            "off_route": off_route or route,   # the route with TOPS_GEMV=0
            "id": "%s-%s%s%s" % (entry, "B%d-" % B if B else "", "x".join(map(str, shape)), "-view" if view else "")}


SUM_CASES = [
    _s("sumRows", (0, 5), "fill"),
    _s("sumRows", (300, 3), "rows"), _s("sumRows", (257,), "rows"), _s("sumRows", (1, 3), "rows"),
    _s("sumRows", (65535,), "rows"), _s("sumRows", (26214, 10), "rows"),
    _s("sumRows", (10,), "rows", B=63), _s("sumRows", (257,), "rows", B=64),
    _s("trace", (300, 300), "rows"),
    _s("sumRows", (257,), "rows", view=True),
] + [_s("sumRows", (n,), "wave", B=B) for B in (64, 66, 67) for n in (1, 63, 64, 65, 256)] + [
    _s("sumRows", (63,), "wave", B=67, view=True),
    _s("sumRows", (4, 64), "cols"), _s("sumRows", (5, 65), "cols"), _s("sumRows", (255, 129), "cols"),
    _s("sumRows", (3, 127), "cols"), _s("sumRows", (5, 65), "cols", B=3),
    _s("sumRows", (5, 65), "cols", view=True),
    _s("sumRows", (256, 64), "two_pass"), _s("sumRows", (4095, 64), "two_pass"), _s("sumRows", (300, 800), "two_pass"),
    _s("batch_sum", (255,), "two_pass", B=1000),
    _s("sumRows", (301, 65), "two_pass", view=True),
    _s("blas_sum", (65536,), "partial"), _s("blas_sum", (70001,), "partial"),
    _s("sumRows", (65536,), "partial"), _s("sumRows", (262143,), "partial"),
    _s("sumRows", (65537,), "partial", view=True),
    _s("sumRows", (4096, 64), "column_sum", off_route="two_pass"),
    _s("sumRows", (26215, 10), "column_sum", off_route="rows"),
    _s("sumRows", (262144,), "column_sum", off_route="partial"),
    _s("batch_sum", (256,), "column_sum", B=1024, off_route="two_pass"),
    _s("sumRows", (26215, 10), "column_sum", view=True, off_route="rows"),
]


def grid_y_case(dtype):
    """the batch in grid.y, past 65,535: [2, 64] a sample in fp32; in fp64 operand and result of that are 101 MB, so one row"""
    return _s("sumRows", (2, 64) if np.dtype(dtype) == np.float32 else (1, 64), "cols", B=65537)


def sum_cases(dtype):
    return SUM_CASES + [grid_y_case(dtype)]


def sum_extra_off_cases(dtype):
    """with TOPS_GEMV=0 only: shapes the column kernel of gemv.hip takes otherwise.  (2048, 8192) is 134 MB in fp64: there the
    same route -- (J + 63) / 64 = 128, so no two-pass -- at half the rows."""
    wide = (2048, 8192) if np.dtype(dtype) == np.float32 else (1024, 8192)
    return [_s("sumRows", (1536, 4096), "column_sum", off_route="two_pass"),
            _s("sumRows", wide, "column_sum", off_route="cols"),
            _s("sumRows", (300000, 10), "column_sum", off_route="rows"),
            _s("sumRows", ((1 << 21) + 17,), "column_sum", off_route="partial")]


def sum_params(case):
    """(O, R, J, sj) of the case's launch_sum_axis call"""
    shape, B = case["shape"], case["B"]
    numel = int(np.prod(shape))
    if case["entry"] == "sumRows":
        return (B if B else 1), shape[0], int(np.prod(shape[1:])), 1
    if case["entry"] == "batch_sum":
        return 1, B, numel, 1
    if case["entry"] == "blas_sum":
        return 1, numel, 1, 0
    if case["entry"] == "trace":
        return 1, shape[0], 1, 0
    raise ValueError(case["entry"])


def sum_case_bytes(case, dtype, gemv_on=True):
    """device bytes of the case: operand (with its NaN surround), result and the route's temporary"""
    n = int(np.prod(case["shape"])) * max(case["B"], 1)
    if case["view"]:
        n += 2 * int(np.prod(case["shape"]))
    O, R, J, _ = sum_params(case)
    route = case["route"] if gemv_on else case["off_route"]
    tmp = {"column_sum": 256 * J, "partial": 1024, "two_pass": two_pass_split(R, J)[0] * J if route == "two_pass" else 0}
    return (n + O * J + tmp.get(route, 0)) * np.dtype(dtype).itemsize


def sum_data(case, dtype, rng, integers=True):
    """host operand, full shape (B leading when batched): integers in -5 .. 5 (every partial sum exact in fp32: at most
    5 * (2^21 + 17) < 2^24) or uniform(-1, 1)"""
    full = ((case["B"],) if case["B"] else ()) + case["shape"]
    if integers:
        return rng.integers(-5, 6, full).astype(dtype)
    return rng.uniform(-1, 1, full).astype(dtype)


def sum_reference(case, x):
    """(float64 result, float64 sum of |x| per result element) from the operand as uploaded"""
    x = np.asarray(x, dtype=np.float64)
    e = case["entry"]
    if e == "sumRows":
        ax = 1 if case["B"] else 0
        return x.sum(axis=ax), np.abs(x).sum(axis=ax)
    if e == "batch_sum":
        return x.sum(axis=0), np.abs(x).sum(axis=0)
    if e == "blas_sum":
        return x.sum(), np.abs(x).sum()
    return np.trace(x), np.abs(np.diagonal(x)).sum()


def run_sum_case(T, Bl, case, x):
    """run the case on backend T (HipT) / Bl (HipB) with host operand x; returns (result as numpy, launches counted)"""
    if case["view"]:
        # [3; shape] (or [B + 2; shape]) NaN everywhere but the middle; the view starts numel elements in
        B = case["B"]
        big = np.full(((B if B else 1) + 2,) + case["shape"], np.nan, dtype=x.dtype)
        big[1:-1] = x if B else x[None]
        d = T.put(big, batched=True)
        dx = T.batch_slice(d, 1, B) if B else T.batch_select(d, 1)
    else:
        dx = T.put(x, batched=bool(case["B"]))
    T.sync()
    before = T.stats()["launches"]
    e = case["entry"]
    if e == "sumRows":
        r = T.sumRows(dx)
    elif e == "batch_sum":
        r = T.batch_sum(dx)
    elif e == "blas_sum":
        r = Bl.sumB(dx)
    else:
        r = Bl.traceB(dx)
    launches = T.stats()["launches"] - before
    return (np.asarray(r) if e in ("blas_sum", "trace") else r.numpy()), launches


# ---- (b) packing a strided view -----------------------------------------------------------------------------------------
# transp of a packed [B;] shape; view: of a batch_select / batch_slice view at a non-zero offset.  A view the restatement
# calls "memcpy" is one packed run, which `contiguous()` recognises first and does not copy at all: the copy's own memcpy
# route is reached by the stack entries that call it directly (test_copy_of_one_packed_run).
def _c(shape, route, B=0, view=False):
    return {"shape": tuple(shape), "B": B, "route": route, "view": view,
            "id": "%s%s%s" % ("B%d-" % B if B else "", "x".join(map(str, shape)), "-view" if view else "")}


COPY_CASES = [
    _c((1, 65), "memcpy"), _c((65, 1), "memcpy"), _c((1, 130), "memcpy", B=3),   # (the last: batch and row merge)
] + [_c(s, "transpose2d") for s in ((63, 64), (64, 65), (65, 63), (130, 64), (64, 130), (65, 130), (130, 63), (63, 130))] + [
    _c((65, 130), "transpose2d", B=1), _c((65, 130), "transpose2d", B=3), _c((63, 65), "transpose2d", B=3),
    _c((65, 63), "transpose2d", view=True), _c((65, 63), "transpose2d", B=3, view=True),
    _c((3, 1, 4), "transpose2d"),            # the unit extent squeezed out: a 4 x 3 transpose
    _c((2, 3, 5, 7), "general"), _c((2, 1, 3, 5), "general"), _c((2, 3, 5), "general", B=3),
    _c((2, 3), "general", B=65536),          # past the batched transpose's grid.z
    _c((7, 5, 3), "general", view=True),
]


def copy_case_view(case):
    return transp_view(case["shape"], case["B"])


def copy_reference(case, x):
    """transp of every sample"""
    x = np.asarray(x)
    if case["B"]:
        return np.ascontiguousarray(np.transpose(x, [0] + list(range(x.ndim - 1, 0, -1))))
    return np.ascontiguousarray(np.transpose(x))


# ---- (c) argMax / argMin --------------------------------------------------------------------------------------------------
ARG_NS = (1, 2, 63, 64, 65, 128, 129, 1000)
ARG_BATCHES = (1, 3, 4, 5, 67)


def arg_rows(n, dtype, seed=0):
    """[K, n] rows: ties, equal rows, signed zeros, infinities, and NaN first / middle / last / at j and j + 64 / several /
    everywhere"""
    rng = np.random.default_rng(1000 * n + seed)
    rows = [rng.integers(-2, 3, n) for _ in range(4)]          # heavy ties
    rows.append(np.full(n, 3.0))
    rows.append(np.zeros(n))
    r = rng.integers(-2, 3, n).astype(np.float64); r[rng.integers(0, n)] = np.inf; rows.append(r)
    r = rng.integers(-2, 3, n).astype(np.float64); r[rng.integers(0, n)] = -np.inf; rows.append(r)
    r = np.full(n, np.inf); r[n // 2] = -np.inf; rows.append(r)
    if n >= 2:
        r = np.zeros(n); r[1::2] = -0.0; rows.append(r)        # [+0, -0, ...]
        r = np.zeros(n); r[0::2] = -0.0; rows.append(r)        # [-0, +0, ...]
    for where in ("first", "middle", "last", "pair", "several", "several", "all", "last_two", "descending"):
        r = rng.integers(-2, 3, n).astype(np.float64)
        if where == "first":
            r[0] = np.nan
        elif where == "middle":
            r[n // 2] = np.nan
        elif where == "last":
            r[n - 1] = np.nan
        elif where == "pair":                                  # the same lane twice
            j = int(rng.integers(0, max(n - 64, 1)))
            r[j] = np.nan
            r[min(j + 64, n - 1)] = np.nan
        elif where == "several":
            r[rng.integers(0, n, 3)] = np.nan
        elif where == "all":
            r[:] = np.nan
        elif where == "last_two":
            r[max(n - 2, 0):] = np.nan
        else:                                                  # 1, NaN, 0.5 stretched: the maximum sits before the NaN
            r = np.linspace(1.0, 0.5, n)
            r[min(1, n - 1)] = np.nan
        rows.append(r)
    return np.array(rows, dtype=dtype)


def arg_reference(rows, minimum=False):
    """`oracle.tensor`'s fold, row by row"""
    O = OTensor(rows.dtype)
    f = O.arg_min if minimum else O.arg_max
    return np.array([f(r) for r in rows], dtype=np.int64)


def arg_closed_form(row, minimum=False):
    """the left fold restarts behind every NaN: n - 1 if the last element is NaN, else the earliest extremum of the suffix
    behind the last NaN"""
    row = np.asarray(row)
    n = len(row)
    nan = np.flatnonzero(np.isnan(row))
    lo = int(nan[-1]) + 1 if len(nan) else 0
    if lo == n:
        return n - 1
    s = row[lo:]
    return lo + int(np.argmin(s) if minimum else np.argmax(s))


def nan_property_rows(count=1000, seed=2024):
    """seeded rows with 1 - 3 NaN each, n out of {1, 2, 3, 63, 64, 65, 128, 129, 200}"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        n = int(rng.choice((1, 2, 3, 63, 64, 65, 128, 129, 200)))
        r = rng.integers(-3, 4, n).astype(np.float64)
        r[rng.integers(0, n, int(rng.integers(1, 4)))] = np.nan
        out.append(r)
    return out


# ---- (d) the rest ---------------------------------------------------------------------------------------------------------
def gather_numels(dtype):
    """row sizes in elements: 4, 8, 12, 16, 20 and 3,136 bytes a row in fp32; 8 (one element), 16, 24 and 3,136 in fp64"""
    return (1, 2, 3, 4, 5, 784) if np.dtype(dtype) == np.float32 else (1, 2, 3, 392)


def gather_indices(n_rows, which, rng):
    if which == "repeated":
        return rng.integers(0, n_rows, 2 * n_rows + 3)
    if which == "reversed":
        return np.arange(n_rows)[::-1].copy()
    return rng.integers(0, n_rows, which)    # a count: 8192 / 8193 straddle the index upload's two paths


STACK_ROWS = (1, 16, 17, 33)
COPY_MANY = ((1, (8,)), (16, (8, 12)), (17, (4, 8)), (3, (8, 5, 12)))   # (pieces, their sizes in elements, cycled); 5: the dword form
ONE_HOT = tuple(itertools.product((1, 10, 1000), (0, 1, 257)))
DIAG = ((2, 1), (2, 5), (2, 300), (3, 1), (3, 5), (3, 150))   # (rank 3 at 300 would be 108 MB in fp32: past MAX_DEVICE_BYTES)
