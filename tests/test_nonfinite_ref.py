"""CPU: tests/nonfinite_ref.py (what the poisoned GPU sweeps of test_gpu_nonfinite.py and tools/poison.py compare against) agrees
with a scalar triple loop in IEEE doubles -- the loop is the definition; the reference only has to be fast at size."""
import numpy as np
import pytest

import nonfinite_ref as NF

POISON = [np.inf, -np.inf, np.nan]


def _loop(a, b, alpha=1.0, beta=0.0, c=None, bias=None):
    M, K = a.shape
    N = b.shape[1]
    out = np.zeros((M, N))
    with np.errstate(invalid="ignore"):
        for i in range(M):
            for j in range(N):
                acc = np.float64(0.0)
                for k in range(K):
                    acc = acc + np.float64(a[i, k]) * np.float64(b[k, j])
                acc = np.float64(alpha) * acc
                if beta != 0.0:
                    acc = acc + np.float64(beta) * np.float64(c[i, j])
                if bias is not None:
                    acc = acc + np.float64(bias[j])
                out[i, j] = acc
    return out


def _poisoned(rng, shape, lo=-2, hi=3):
    x = rng.integers(lo, hi, shape).astype(np.float64)
    for _ in range(int(rng.integers(0, 4))):      # up to three poisoned entries
        x[tuple(int(rng.integers(0, s)) for s in shape)] = POISON[int(rng.integers(0, 3))]
    return x


def test_contract_is_the_triple_loop_on_small_poisoned_cases():
    rng = np.random.default_rng(0x6e66)
    nonfinite = 0
    for _ in range(400):
        M, K, N = (int(v) for v in rng.integers(1, 9, 3))
        a, b = _poisoned(rng, (M, K)), _poisoned(rng, (K, N))
        want = _loop(a, b)
        got = NF.contract(a, b)
        assert NF.same_class_and_value(got, want), (a, b, got, want)
        nonfinite += int((~np.isfinite(want)).sum())
    assert nonfinite > 400       # (the cases do exercise the classes)


def test_the_alpha_beta_bias_form_is_the_triple_loop():
    rng = np.random.default_rng(0x6e67)
    for case in range(300):
        M, K, N = (int(v) for v in rng.integers(1, 9, 3))
        a, b = _poisoned(rng, (M, K)), _poisoned(rng, (K, N))
        c, bias = _poisoned(rng, (M, N), -4, 5), _poisoned(rng, (N,), -3, 4)
        alpha = float(rng.choice([1.0, 2.0, -2.0, -1.0]))
        beta = float(rng.choice([0.0, 3.0, -3.0, 1.0]))
        use_bias = bool(rng.integers(2))
        want = _loop(a, b, alpha, beta, c, bias if use_bias else None)
        got = NF.contract_epilogue(a, b, alpha, beta, c, bias if use_bias else None)
        assert NF.same_class_and_value(got, want), (case, alpha, beta, got, want)


def test_beta_zero_does_not_read_c():
    """the BLAS convention, deliberately not IEEE (0 * NaN would be NaN): beta == 0 means C is not an input"""
    a, b = np.array([[1.0, 2.0]]), np.array([[3.0], [4.0]])
    c = np.array([[np.nan]])
    assert NF.contract_epilogue(a, b, 1.0, 0.0, c)[0, 0] == 11.0
    assert np.isnan(NF.contract_epilogue(a, b, 1.0, 1.0, c)[0, 0])


def test_k_of_one():
    a = np.array([[np.inf], [2.0], [0.0], [np.nan], [-np.inf]])
    b = np.array([[3.0, 0.0, -1.0, np.inf, np.nan]])
    want = _loop(a, b)
    got = NF.contract(a, b)
    assert NF.same_class_and_value(got, want)
    assert got[0, 0] == np.inf and np.isnan(got[0, 1]) and got[0, 2] == -np.inf and got[0, 3] == np.inf and np.isnan(got[0, 4])
    assert got[1].tolist()[:4] == [6.0, 0.0, -2.0, np.inf] and np.isnan(got[2, 3]) and got[4, 3] == -np.inf
    assert np.isnan(got[3]).all()


def test_a_row_of_nothing_but_nan():
    rng = np.random.default_rng(3)
    a = rng.integers(-2, 3, (5, 7)).astype(np.float64)
    b = rng.integers(-2, 3, (7, 6)).astype(np.float64)
    a[2, :] = np.nan
    got = NF.contract(a, b)
    assert np.isnan(got[2]).all()
    assert np.array_equal(np.delete(got, 2, axis=0), np.delete(a, 2, axis=0) @ b)
    assert NF.same_class_and_value(got, _loop(a, b))


def test_both_infinities_meeting_in_one_output():
    a = np.array([[np.inf, 1.0, -np.inf], [np.inf, 1.0, np.inf], [np.inf, 1.0, 2.0]])
    b = np.array([[1.0, 2.0], [5.0, 5.0], [1.0, -3.0]])
    got = NF.contract(a, b)
    # row 0: inf - inf, inf + inf;  row 1: inf + inf, inf - inf;  row 2: inf + finite
    assert np.isnan(got[0, 0]) and got[0, 1] == np.inf
    assert got[1, 0] == np.inf and np.isnan(got[1, 1])
    assert got[2, 0] == np.inf and got[2, 1] == np.inf
    assert NF.same_class_and_value(got, _loop(a, b))
    # an infinity in each operand at the same k: inf * -inf = -inf
    a2, b2 = np.array([[np.inf, 1.0]]), np.array([[-np.inf], [4.0]])
    assert NF.contract(a2, b2)[0, 0] == -np.inf


def test_sum_rows_and_the_comparison_itself():
    x = np.array([[1.0, np.inf, np.inf, np.nan], [2.0, 3.0, -np.inf, 1.0]])
    got = NF.sum_rows(x)
    assert got[0] == 3.0 and got[1] == np.inf and np.isnan(got[2]) and np.isnan(got[3])
    w = np.array([0.0, np.inf, -np.inf, np.nan, 5.0])
    assert NF.same_class_and_value(np.array([-0.0, np.inf, -np.inf, np.nan, 5.0]), w)      # (the sign of a zero is not compared)
    for bad in ([0.0, np.inf, np.inf, np.nan, 5.0], [0.0, np.inf, -np.inf, 1.0, 5.0], [np.nan, np.inf, -np.inf, np.nan, 5.0],
                [0.0, 1e38, -np.inf, np.nan, 5.0], [0.0, np.inf, -np.inf, np.nan, 5.0000001]):
        assert not NF.same_class_and_value(np.array(bad), w), bad
    assert not NF.same_class_and_value(w[:4], w)
    assert NF.same_class_and_value(w.astype(np.float32), w)
