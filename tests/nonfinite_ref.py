"""The IEEE value of a contraction whose operands are exact small integers except for some +-inf / NaN entries, without asking a
BLAS what it thinks of `0 * inf` (pure numpy; tests/test_nonfinite_ref.py holds it against a scalar triple loop).

A sum of products is NaN when any product is NaN (`NaN * x`, `inf * 0`) or when +inf and -inf both occur among the products;
it is +-inf when only that sign occurs; otherwise it is the finite sum.  None of that depends on the order of the additions,
so one reference serves every route, split and stream-K order.  The finite part is an fp64 product with the non-finite entries
replaced by zero (exact on small integers); the class of each output comes from indicator-matrix products that COUNT the NaN,
+inf and -inf contributions (counts of at most K: exact in fp64)."""
import numpy as np


def _f64(x):
    return np.asarray(x, dtype=np.float64)


def _class_counts(a, b):
    """(NaN count, +inf count, -inf count) among the products a[i, k] b[k, j] of each output, dense"""
    f = lambda m: m.astype(np.float64)
    nan_a, nan_b, inf_a, inf_b = np.isnan(a), np.isnan(b), np.isinf(a), np.isinf(b)
    # a NaN product: a NaN factor, or an infinity opposite a zero
    n_nan = f(nan_a) @ np.ones(b.shape) + f(~nan_a) @ f(nan_b) + f(inf_a) @ f(b == 0) + f(a == 0) @ f(inf_b)
    # an infinite product: at least one infinite factor, the other one positive or negative (an infinity included)
    pa, na, pb, nb = a > 0, a < 0, b > 0, b < 0          # (comparisons with NaN are False)
    fin_pa, fin_na = pa & ~inf_a, na & ~inf_a            # (finite a: the infinity has to be b's)
    n_pos = f(pa & inf_a) @ f(pb) + f(na & inf_a) @ f(nb) + f(fin_pa) @ f(pb & inf_b) + f(fin_na) @ f(nb & inf_b)
    n_neg = f(pa & inf_a) @ f(nb) + f(na & inf_a) @ f(pb) + f(fin_pa) @ f(nb & inf_b) + f(fin_na) @ f(pb & inf_b)
    return n_nan, n_pos, n_neg


def _counts(a, b):
    """(finite part, NaN count, +inf count, -inf count) of sum_k a[i, k] b[k, j], each (M, N).  A product is non-finite only in
    the rows of a and the columns of b that hold a non-finite entry: the indicator products run on those alone."""
    a, b = _f64(a), _f64(b)
    assert a.ndim == 2 and b.ndim == 2 and a.shape[1] == b.shape[0], (a.shape, b.shape)
    fin = np.where(np.isfinite(a), a, 0.0) @ np.where(np.isfinite(b), b, 0.0)
    counts = [np.zeros(fin.shape) for _ in range(3)]
    rows = np.nonzero(~np.isfinite(a).all(axis=1))[0]
    cols = np.nonzero(~np.isfinite(b).all(axis=0))[0]
    if len(rows):
        for c, v in zip(counts, _class_counts(a[rows], b)):
            c[rows, :] = v
    if len(cols):
        for c, v in zip(counts, _class_counts(a, b[:, cols])):
            c[:, cols] = v
    return (fin,) + tuple(counts)


def _split(x):
    """the same four for a plain array: an element is its own single contribution"""
    x = _f64(x)
    f = lambda m: m.astype(np.float64)
    return np.where(np.isfinite(x), x, 0.0), f(np.isnan(x)), f(x == np.inf), f(x == -np.inf)


def _join(fin, n_nan, n_pos, n_neg):
    out = np.array(fin, dtype=np.float64, copy=True)
    out[n_pos > 0] = np.inf
    out[n_neg > 0] = -np.inf
    out[(n_nan > 0) | ((n_pos > 0) & (n_neg > 0))] = np.nan
    return out


def _scaled(s, parts):
    """s * x for a finite non-zero scalar s: the class stays, a negative s swaps the infinities"""
    assert np.isfinite(s) and s != 0.0, s
    fin, n_nan, n_pos, n_neg = parts
    return (s * fin, n_nan, n_pos, n_neg) if s > 0 else (s * fin, n_nan, n_neg, n_pos)


def contract(a, b):
    """sum_k a[i, k] b[k, j] in IEEE arithmetic, fp64"""
    return _join(*_counts(a, b))


def contract_epilogue(a, b, alpha=1.0, beta=0.0, c=None, bias=None):
    """alpha * (a . b) + beta * c + bias[n].  alpha is finite and non-zero.  beta == 0 does NOT read c (the BLAS convention:
    a poisoned c must not reach the output then)."""
    parts = [_scaled(alpha, _counts(a, b))]
    if beta != 0.0:
        parts.append(_scaled(beta, _split(c)))
    if bias is not None:
        parts.append(tuple(np.broadcast_to(p[None, :], parts[0][0].shape) for p in _split(bias)))
    return _join(*[sum(p[i] for p in parts) for i in range(4)])


def sum_rows(x):
    """out[j] = sum_i x[i, j] (`sumRows`: the contraction with no vector, i.e. with a row of ones -- every element is its own
    contribution, so the counts are plain column counts)"""
    x = np.asarray(x)
    fin = np.where(np.isfinite(x), x, 0).sum(axis=0, dtype=np.float64)
    return _join(fin, np.isnan(x).sum(axis=0), (x == np.inf).sum(axis=0), (x == -np.inf).sum(axis=0))


def same_class_and_value(got, want):
    """The NaN masks are equal, the +inf masks are equal, the -inf masks are equal, and every other element is equal with ==
    (so the sign of a zero is not compared: accumulators start at +0)."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return False
    g, w = got.astype(np.float64), want.astype(np.float64)
    if not (np.array_equal(np.isnan(g), np.isnan(w)) and np.array_equal(g == np.inf, w == np.inf)
            and np.array_equal(g == -np.inf, w == -np.inf)):
        return False
    fin = np.isfinite(w)
    return bool(np.all(g[fin] == w[fin]))


def describe(got, want, limit=6):
    """a few of the elements on which same_class_and_value fails, for an assertion's message"""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return "shape %s against %s" % (got.shape, want.shape)
    g, w = got.astype(np.float64), want.astype(np.float64)
    bad = ~((g == w) | (np.isnan(g) & np.isnan(w)))
    idx = np.argwhere(bad)
    return "%d of %d differ: %s" % (len(idx), g.size, [(tuple(int(v) for v in i), float(g[tuple(i)]), float(w[tuple(i)])) for i in idx[:limit]])
