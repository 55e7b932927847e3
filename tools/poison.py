"""FUZZ_POISON=1: the contraction sweeps (gemm_fuzz, route_fuzz, pinned_fuzz, kw16_check, t32_check, learn_check, gmul_fuzz,
kw_epilogue_fuzz, pinned_epilogue_check) run every case twice -- once with +-inf / NaN placed in the operands where a kernel that
loads beyond an extent and trusts `x * 0` would turn them into a NaN that IEEE does not allow, once more with the clean
integer operands on the same shape (the split-K / stream-K / wave-split workspaces then still hold the poisoned run's partial
tiles: a reduction that reads a slot nobody wrote this time shows up as NaN).

The poison comes from a generator of its own, so the tool's sequence of extents, layouts and beta choices -- hence the route of
every case -- is the one of the integer run.  The reference is tests/nonfinite_ref.py (class by counting; no BLAS is asked about
0 * inf).  A case whose reference has no non-finite output, or (M, N >= 8) less than half finite ones, is an ERROR, never a skip.

Without the variable nothing here changes what a tool does: `rounds` yields the operands once, `want_*` / `same` are not called.
Test infrastructure; nothing in the product imports it."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import nonfinite_ref as NF  # noqa: E402

ON = os.environ.get("FUZZ_POISON") == "1"
VALUES = (np.inf, -np.inf, np.nan)
KINDS = ("k-ends", "last-row-col", "k-tile", "zero-opposite")
_rng = np.random.default_rng(0x706F6973)      # NOT the tool's generator
stats = {"poisoned": 0, "nonfinite": 0, "clean": 0, "kinds": {k: 0 for k in KINDS}}


def draw(rng=None, inf_only=False):
    """one poison value (+inf, -inf or NaN) from the poison generator, or from the generator given"""
    rng = _rng if rng is None else rng
    return VALUES[int(rng.integers(2 if inf_only else 3))]


def integers(*args, rng=None):
    """a placement index from the poison generator (the tools never draw a placement from their own)"""
    return int((_rng if rng is None else rng).integers(*args))


def pair(a, b, kind=None, rng=None):
    """Poisoned copies of a (M, K) and b (K, N): at most two rows of a and two columns of b, so most of the output stays finite."""
    rng = _rng if rng is None else rng
    val = lambda inf_only=False: draw(rng, inf_only)
    a, b = np.array(a, copy=True), np.array(b, copy=True)
    (M, K), N = a.shape, b.shape[1]
    kind = KINDS[int(rng.integers(len(KINDS)))] if kind is None else kind
    stats["kinds"][kind] += 1
    m, n = int(rng.integers(M)), int(rng.integers(N))
    if kind == "k-ends":          # the first and the last k of a row (k-contiguous: the element after a row's tail is the next row's k = 0)
        a[m, 0] = val(); a[m, K - 1] = val()
        b[0, n] = val(); b[K - 1, n] = val()
        if M > 1 and rng.integers(2):
            a[(m + 1) % M, 0] = val()
    elif kind == "last-row-col":  # what clamped edge lanes re-read
        a[M - 1, :] = val()
        b[:, N - 1] = val()
    elif kind == "k-tile":        # the first k beyond the last whole k-tile of 16 and of 32 (a whole multiple: the last tile's first k)
        k16, k32 = [(K // u) * u if K % u else max(K - u, 0) for u in (16, 32)]
        m2, n2 = int(rng.integers(M)), int(rng.integers(N))
        a[m, k16] = val(); a[m2, k32] = val()
        b[k32, n] = val(); b[k16, n2] = val()
    else:                         # a zero opposite an infinity: inf * 0 = NaN is demanded there, and forbidden everywhere else
        k, k2 = int(rng.integers(K)), int(rng.integers(K))
        n0, m0 = int(rng.integers(N)), int(rng.integers(M))
        b[k, n0] = 0
        if N > 1 and b[k, (n0 + 1) % N] == 0:
            b[k, (n0 + 1) % N] = 1
        a[m0, k2] = 0
        a[m, k] = val(inf_only=True)
        if not (k2 == k and n == n0):
            b[k2, n] = val(inf_only=True)
    return a, b


def rounds(a, b):
    """The operand pairs a case runs with: the tool's own once; under FUZZ_POISON=1 the poisoned pair, then the clean one."""
    if not ON:
        yield a, b
        return
    yield pair(a, b)
    yield a, b


def check_case(want, M, N):
    """the per-case conditions of a poisoned round (from the reference, on the CPU)"""
    fin = np.isfinite(want)
    if fin.all():
        raise RuntimeError("poison: a case of %d x %d whose reference output is all finite" % (M, N))
    if M >= 8 and N >= 8 and 2 * int(fin.sum()) < fin.size:
        raise RuntimeError("poison: %d of %d reference outputs finite at %d x %d" % (int(fin.sum()), fin.size, M, N))


def reference(a, b, alpha=1.0, beta=0.0, c=None, bias=None):
    return NF.contract_epilogue(a, b, alpha, beta, c, bias)


def count(want, M, N, poisoned):
    """a poisoned round is counted and held to the per-case conditions; a clean one is counted"""
    if poisoned:
        stats["poisoned"] += 1
        stats["nonfinite"] += int(not np.isfinite(want).all())      # (counted from the reference itself ...)
        check_case(want, M, N)                                      # (... and a case without one is an error)
    else:
        stats["clean"] += 1


def want_product(a, b, dtype, alpha=1.0, beta=0.0, c=None, bias=None):
    """the reference of either round, in the element type"""
    want = reference(a, b, alpha, beta, c, bias)
    count(want, a.shape[0], b.shape[1], not (np.isfinite(a).all() and np.isfinite(b).all()))
    return want.astype(dtype)


def same(got, want):
    """np.array_equal on a clean round; equal NaN / +inf / -inf masks and == elsewhere on a poisoned one"""
    got, want = np.asarray(got), np.asarray(want)
    if np.isfinite(want).all():
        return got.shape == want.shape and np.array_equal(got, want)
    ok = NF.same_class_and_value(got, want)
    if not ok:
        sys.stderr.write("POISON MISMATCH %s\n" % NF.describe(got, want))
    return ok


def close(got, ref, tol):
    """an activation's values: NaN exactly where the fp64 reference is NaN, within tol everywhere else (logistic(+-inf) = 1 / 0 and
    tanh(+-inf) = +-1 are finite values of the reference)"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    if got.shape != ref.shape or not np.array_equal(np.isnan(got), np.isnan(ref)):
        return False
    ok = ~np.isnan(ref)
    return bool(np.all(np.abs(got[ok] - ref[ok]) < tol))


def logistic(z):
    with np.errstate(over="ignore"):
        return 1 / (1 + np.exp(-np.asarray(z, dtype=np.float64)))


def report(tool):
    if ON:
        print("poison %s: poisoned cases %d, with non-finite reference outputs %d, skipped 0, clean reruns %d, placements %s"
              % (tool, stats["poisoned"], stats["nonfinite"], stats["clean"], stats["kinds"]), flush=True)
