"""Case tables and the float64 reference for the row heads (test infrastructure; imports no GPU code).  A row head is the
per-row code behind a stack's last contraction: a row of logits z and a target row y become softmax or logistic outputs, the
cotangent dz and the row's loss.  tests/test_head_cases.py checks the tables on the CPU, tests/test_gpu_heads.py runs every
head of the library on them.

The reference is plain numpy in float64 on the operands AS STORED in the element type under test (`stored`), evaluated
literally: a -inf logit under a zero target is 0 * inf = NaN here as in the reference's own arithmetic, and the class of every
output (NaN, +inf, -inf, finite) of a special row is whatever these few lines give.

Every logit row is built in float64 and rounded to the element type before anything looks at it, so it is exact in both: the
GPU tests hand the rows to the heads bit for bit (identity weights times a power of two, or the bias)."""
import numpy as np

DTYPES = (np.float32, np.float64)
# exp(-x) is exactly zero beyond this spread whether or not denormals are flushed: 149 ln 2 and 1074 ln 2
EXP_RANGE = {np.float32: 149 * np.log(2.0), np.float64: 1074 * np.log(2.0)}
# 0 and 30: nothing underflows; 100: denormal p in fp32; 120: beyond fp32's range; 1000: beyond fp64's; 1e30: z - max still finite
SPREADS = (0.0, 30.0, 100.0, 120.0, 1000.0, 1e30)
PATTERNS = ("equal", "dominant", "two_max", "ramp")
TARGETS = ("onehot", "soft1", "soft_half", "zero", "soft3")   # (soft3 last: a batch of one row gets a target with dz far from 0)
TARGET_SUM = {"onehot": 1.0, "soft1": 1.0, "soft_half": 0.5, "zero": 0.0, "soft3": 3.0}
BATCHES = (7, 7, 5, 1)          # how a spread's 20 rows go out: a second workgroup, a partly filled one, a single row
# each head's own edges
WIDTHS = {
    "fused": (1, 2, 10, 16),                      # gemm_small.hip: one 16-wide tile
    "rows": (17, 63, 64, 65, 130),                # loss_grad_rows / infer_rows: the lane loop's tail, a third pass
    "narrow": (8, 9, 16, 17, 32),                 # infer_narrow: NP 8 / 16 / 32
    "recon": (3, 64, 65, 1024, 1028, 1031),       # recon_head.hip: pieces, the element path, a second tile
    "wave": (1, 10, 17, 63, 64),                  # induce_seq.hip: the head is one wave, at most 64 wide
}
SE_SPREADS = (0.0, 30.0, 100.0, 120.0, 1000.0)    # squared-error heads: (z - t)^2 has to stay finite in fp32


def stored(x, dt):
    """x as the element type holds it, in float64"""
    return np.asarray(x, dtype=dt).astype(np.float64)


# ---- the reference -----------------------------------------------------------------------------------------------------------
def softmax_ce(z, y):
    """(p, dz, loss) of softmax >>> crossEntropy over the last axis, on lse = log sum exp(z - max z)"""
    z, y = np.asarray(z, np.float64), np.asarray(y, np.float64)
    with np.errstate(all="ignore"):
        d = z - z.max(axis=-1, keepdims=True)
        lse = np.log(np.exp(d).sum(axis=-1, keepdims=True))
        p = np.exp(d - lse)
        dz = p * y.sum(axis=-1, keepdims=True) - y
        loss = (y * (lse - d)).sum(axis=-1)
    return p, dz, loss


def softmax_ce_literal(z, y):
    """the loss as -sum y log softmax(z), the softmax with the row maximum subtracted: what softmax_ce is held against"""
    z, y = np.asarray(z, np.float64), np.asarray(y, np.float64)
    with np.errstate(all="ignore"):
        e = np.exp(z - z.max(axis=-1, keepdims=True))
        return -(y * np.log(e / e.sum(axis=-1, keepdims=True))).sum(axis=-1)


def _se(a, da, y):
    d = a - np.asarray(y, np.float64)
    return a, 2.0 * d * da, (d * d).sum(axis=-1)


def logistic_se(z, y):
    """(a, dz, loss) of logistic >>> squaredError (recon_head.hip, pair 2): dz = 2 (a - t) a (1 - a)"""
    with np.errstate(all="ignore"):
        a = 1.0 / (1.0 + np.exp(-np.asarray(z, np.float64)))
        return _se(a, a * (1.0 - a), y)


def tanh_se(z, y):
    """pair 3: dz = 2 (a - t) (1 - a^2)"""
    with np.errstate(all="ignore"):
        a = np.tanh(np.asarray(z, np.float64))
        return _se(a, 1.0 - a * a, y)


def identity_se(z, y):
    """pair 4: dz = 2 (a - t)"""
    with np.errstate(all="ignore"):
        a = np.asarray(z, np.float64)
        return _se(a, np.ones_like(a), y)


HEADS = {"softmax": softmax_ce, "logistic": logistic_se, "tanh": tanh_se, "identity": identity_se}


def klass(x):
    """0 finite, 1 NaN, 2 +inf, 3 -inf, elementwise"""
    x = np.asarray(x, np.float64)
    return np.where(np.isnan(x), 1, np.where(x == np.inf, 2, np.where(x == -np.inf, 3, 0)))


# ---- the rows ----------------------------------------------------------------------------------------------------------------
def _ramp_frac(n):
    j = np.arange(n)
    if n <= 9:
        return np.round(8.0 * j / max(n - 1, 1)) / 8.0     # 0 .. 1 in eighths, the largest at n - 1
    return (j % 9) / 8.0                                    # the largest at 8, again at 17, 26, ...: argMax takes the earliest


def logits(pattern, spread, n, dt):
    """a row of n logits between -spread / 2 and +spread / 2, as stored in dt (float64)"""
    lo, hi = -0.5 * spread, 0.5 * spread
    if pattern == "equal":
        z = np.full(n, hi)
    elif pattern == "dominant":
        z = np.full(n, lo)
        z[(2 * n) // 3] = hi
    elif pattern == "two_max":
        z = np.full(n, lo)
        z[n // 3] = hi
        z[n - 1] = hi
    elif pattern == "ramp":
        z = lo + spread * _ramp_frac(n)
    else:
        raise ValueError(pattern)
    return stored(z, dt)


def _dense(n, hot, total):
    """n small dyadic numbers, none zero, summing to `total` exactly: 1 / q each, the rest on `hot`"""
    q = 2.0 ** int(np.ceil(np.log2(2 * n)))
    y = np.full(n, 1.0 / q)
    y[hot] += 1.0 - n / q
    return total * y


def target(kind, n, k):
    """target row number k of a kind; exact in both element types"""
    hot = (3 * k + 1) % n
    if kind == "onehot":
        y = np.zeros(n)
        y[hot] = 1.0
        return y
    if kind == "zero":
        return np.zeros(n)
    return _dense(n, hot, TARGET_SUM[kind])


def finite_cases(n, dt, spreads=SPREADS):
    """every pattern x spread x target at width n: dicts id, z, y, spread (of the stored row), underflow (some p is exactly
    zero in dt).  Spread-major, then target, then pattern: a batch of neighbours shares a scale."""
    out = []
    for s in spreads:
        k = 0
        for tk in TARGETS:
            for pat in PATTERNS:
                z = logits(pat, s, n, dt)
                sp = float(z.max() - z.min())
                out.append({"id": "%s-%g-%s-n%d" % (pat, s, tk, n), "pattern": pat, "target": tk, "nominal": s, "z": z,
                            "y": target(tk, n, k), "spread": sp, "underflow": sp > EXP_RANGE[dt],
                            "tie_free": int((z == z.max()).sum()) == 1})
                k += 1
    return out


def batches(cases, sizes=BATCHES):
    """the cases in order, cut into batches of the sizes in turn"""
    out, i, k = [], 0, 0
    while i < len(cases):
        b = sizes[k % len(sizes)]
        out.append(cases[i:i + b])
        i += b
        k += 1
    return out


def special_batches(n, dt):
    """The rows whose outputs are non-finite by arithmetic.  Each entry: id, x (finite rows, [B, n]), bias ([n]: where a
    non-finite LOGIT comes from -- it is shared by the rows of a batch), y ([B, n]: where a non-finite TARGET comes from) and
    loss_class (klass of each row's loss).  z = x + bias."""
    j = n // 2
    x = np.stack([logits("ramp", 30.0, n, dt), logits("dominant", 30.0, n, dt), logits("equal", 30.0, n, dt),
                  logits("two_max", 30.0, n, dt), logits("ramp", 30.0, n, dt)])
    hot_j, hot_other = np.zeros(n), np.zeros(n)
    hot_j[j] = 1.0
    hot_other[(j + 1) % n] = 1.0
    ys = np.stack([hot_other, _dense(n, j, 1.0), np.zeros(n), hot_j, _dense(n, (j + 1) % n, 3.0)])
    zero = np.zeros(n)

    def at_j(v):
        b = np.zeros(n)
        b[j] = v
        return b

    out = [
        {"id": "nan_logit-n%d" % n, "x": x, "bias": at_j(np.nan), "y": ys, "loss_class": [1] * 5},
        {"id": "pinf_logit-n%d" % n, "x": x, "bias": at_j(np.inf), "y": ys, "loss_class": [1] * 5},       # inf - inf
        {"id": "all_ninf-n%d" % n, "x": x, "bias": np.full(n, -np.inf), "y": ys, "loss_class": [1] * 5},  # inf - inf again
    ]
    if n >= 2:
        # a -inf logit: p = 0 there and dz is finite; the loss is 0 * inf = NaN under a zero target (rows 0 and 2), +inf under
        # any other
        out.append({"id": "ninf_logit-n%d" % n, "x": x, "bias": at_j(-np.inf), "y": ys, "loss_class": [1, 2, 1, 2, 2]})
    yn = ys.copy()
    yn[3, (j + 1) % n] = np.nan        # a NaN target: that row's dz and loss, no other row
    out.append({"id": "nan_target-n%d" % n, "x": x, "bias": zero, "y": yn, "loss_class": [0, 0, 0, 1, 0]})
    for c in out:
        c["x"], c["bias"], c["y"] = stored(c["x"], dt), stored(c["bias"], dt), stored(c["y"], dt)
    return out
