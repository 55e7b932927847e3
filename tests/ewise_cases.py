"""Case tables, the routing restatement and the references for the elementwise kernels behind `to_lift` (csrc/ewise.hip,
csrc/expr.cpp, csrc/expr_jit.cpp).  Test infrastructure: imports no GPU code.  tests/test_ewise_cases.py checks the tables
and the references on the CPU, tests/test_gpu_ewise_routes.py runs them.

`ew_plan` restates the routing decision of `to::ew_plan`; every ROUTE_CASES entry carries the cell it is meant to reach,
the CPU test checks the annotation against the restatement and the GPU test the restatement against the library
(`to_ewise_route_query`).  `RULES` states, per opcode, what the library computes -- the reference of the GPU tests is an
interpreter of the SSA program over these rules in `np.longdouble` (`ssa_eval`), so it is the same for the pre-fused
functors, the run-time specialised kernels and the bytecode VM.

Left out of ROUTE_CASES on purpose (both are past the few-seconds budget of a test): the functor route's second piece with
two or more inputs (its cap is one piece a thread up to 2^20 blocks: more than 4 GiB of fp32 output) and the
`totalv > 2^25` cap formula of the one-input functor route (more than 512 MiB)."""
import numpy as np

(X_CONST, X_ADD, X_SUB, X_MUL, X_DIV, X_NEG, X_RECIP, X_EXP, X_LOG, X_SQRT, X_ABS, X_SIGNUM, X_SIN, X_COS, X_TANH, X_POW,
 X_MAX, X_MIN) = range(18)
OPS = {"const": X_CONST, "add": X_ADD, "sub": X_SUB, "mul": X_MUL, "div": X_DIV, "neg": X_NEG, "recip": X_RECIP, "exp": X_EXP,
       "log": X_LOG, "sqrt": X_SQRT, "abs": X_ABS, "signum": X_SIGNUM, "sin": X_SIN, "cos": X_COS, "tanh": X_TANH, "pow": X_POW,
       "max": X_MAX, "min": X_MIN}
OP_NAMES = {v: k for k, v in OPS.items()}
UNARY = ("neg", "recip", "exp", "log", "sqrt", "abs", "signum", "sin", "cos", "tanh")
BINARY = ("add", "sub", "mul", "div", "pow", "max", "min")
DTYPES = (np.float32, np.float64)
DT_IDS = ("f32", "f64")
TOL = {np.float32: 1e-5, np.float64: 1e-12}        # tools/expr_fuzz.py's band; 1e-12 is the README's fp64 figure
# expression kinds (to_expr_kind): pre-fused functors by number, 100 = specialised at run time, 0 = bytecode VM
KIND = {"affine": 1, "mul": 2, "exp": 3, "log": 4, "recip": 5, "logistic": 6, "d_logistic": 7, "tanh": 8, "sqrt": 9, "div": 10,
        "d_tanh": 13, "jit": 100, "vm": 0}


# ---- the routing rule ---------------------------------------------------------------------------------------------------------
STREAM_BYTES = 64 << 20
BLOCK = 256
CAP = 2048


def vlen(dtype):
    return 16 // np.dtype(dtype).itemsize


def ew_plan(dtype, n_inputs, total, aligned, periods, family):
    """(form, blocks, wraps?, second piece?) of one elementwise launch: `to::ew_plan` restated.  wraps: some thread makes a
    second trip of its grid-stride loop."""
    if total <= 0:
        return ("scalar", 0, False, False)
    esz, V = np.dtype(dtype).itemsize, vlen(dtype)
    periods = [total] * n_inputs if periods is None else list(periods)
    vec = family != "vm" and aligned and total % V == 0 and all(p % V == 0 for p in periods)
    if not vec:
        blocks = min((total + BLOCK - 1) // BLOCK, CAP)
        return ("scalar", blocks, total > blocks * BLOCK, False)
    totalv = total // V
    streaming = total * esz >= STREAM_BYTES
    if not streaming:
        cap = CAP
    elif family == "jit":
        cap = 32768
    elif n_inputs >= 2:
        cap = min((totalv + 255) // 256, 1 << 20)
    else:
        cap = 32768 if totalv <= (1 << 25) else min((totalv + 511) // 512, 1 << 20)
    blocks = min((totalv + BLOCK - 1) // BLOCK, cap)
    if streaming and totalv >= (1 << 20):
        return ("stream", blocks, totalv > 2 * blocks * BLOCK, totalv > blocks * BLOCK)
    return ("vec", blocks, totalv > blocks * BLOCK, False)


def _r(name, family, n, total, form, wrap=False, second=False, only=None):
    """total: a function of V (elements per 16-byte piece)"""
    return {"id": "%s-%s-n%d" % (family, name, n), "family": family, "n": n, "total": total, "form": form, "wrap": wrap,
            "second": second, "only": only}


def _route_rows(family, second_n2):
    rows = [
        _r("scalar", family, 1, lambda V: 1003, "scalar"),
        _r("scalar", family, 2, lambda V: 1003, "scalar"),
        _r("scalar-edge", family, 1, lambda V: CAP * BLOCK - 1, "scalar"),                  # the last size without a wrap
        _r("scalar-wrap", family, 1, lambda V: CAP * BLOCK + 3, "scalar", wrap=True),
        _r("scalar-wrap", family, 2, lambda V: CAP * BLOCK + 3, "scalar", wrap=True),
        _r("vec", family, 1, lambda V: V * 1000, "vec"),
        _r("vec", family, 2, lambda V: V * 1000, "vec"),
        _r("vec-edge", family, 1, lambda V: V * CAP * BLOCK, "vec"),
        _r("vec-wrap", family, 1, lambda V: V * CAP * BLOCK + V, "vec", wrap=True),
        _r("vec-wrap", family, 2, lambda V: V * CAP * BLOCK + V, "vec", wrap=True),
        _r("vec-below-stream", family, 1, lambda V: V * ((1 << 22) - 1), "vec", wrap=True),   # one piece under 64 MiB
        _r("stream", family, 1, lambda V: V * (1 << 22), "stream"),                          # 64 MiB exactly
        _r("stream", family, 2, lambda V: V * (1 << 22), "stream"),
        # 128 MiB + 16 KB: exactly the first 1000 threads take a second piece, the ragged tail of the trip
        _r("stream-second", family, 1, lambda V: V * ((1 << 23) + 1000), "stream", second=True,
           only=None if family == "jit" else np.float32),
    ]
    if second_n2:
        rows.append(_r("stream-second", family, 2, lambda V: V * ((1 << 23) + 1000), "stream", second=True))
    return rows


ROUTE_CASES = _route_rows("functor", False) + _route_rows("jit", True) + [
    _r("scalar", "vm", 1, lambda V: 1003, "scalar"),
    _r("scalar", "vm", 2, lambda V: V * 1000, "scalar"),          # what the other families would vectorise
    _r("scalar-edge", "vm", 2, lambda V: CAP * BLOCK, "scalar"),
    _r("scalar-wrap", "vm", 2, lambda V: CAP * BLOCK + 3, "scalar", wrap=True),
]
# the cells the issue asks for: (family, form, wrap, second, n)
REQUIRED_CELLS = (
    [(f, "scalar", False, False, None) for f in ("functor", "jit", "vm")] + [(f, "scalar", True, False, None) for f in ("functor", "jit", "vm")] +
    [(f, "vec", w, False, None) for f in ("functor", "jit") for w in (False, True)] +
    [(f, "stream", False, False, n) for f in ("functor", "jit") for n in (1, 2)] +
    [("functor", "stream", False, True, 1), ("jit", "stream", False, True, 1), ("jit", "stream", False, True, 2)])


def route_cases(dtype, family=None):
    return [c for c in ROUTE_CASES if (c["only"] is None or c["only"] == dtype) and (family is None or c["family"] == family)]


def case_total(case, dtype):
    return case["total"](vlen(dtype))


# periods: (B, numel of the unbatched operands); which operand is batched is the program's business
PERIOD_BATCHES = (1, 2, 3, 5)
PERIOD_NUMELS = (1, 2, 3, 4, 6, 8, 12)


# ---- SSA programs -------------------------------------------------------------------------------------------------------------
class Prog:
    """an SSA program as to_expr_compile takes it: value v < arity is input v, value arity + i instruction i's result"""

    def __init__(self, arity, name=""):
        self.arity, self.code, self.consts, self.name = arity, [], [], name

    def k(self, c):
        self.consts.append(float(c))
        self.code.append((X_CONST, len(self.consts) - 1, 0))
        return self.arity + len(self.code) - 1

    def op(self, name, a, b=None):
        self.code.append((OPS[name], a, a if b is None else b))
        return self.arity + len(self.code) - 1

    def unclassified(self):
        """the same function behind `max r r` (the identity on every value, NaN and -0.0 included): the classifier leaves
        programs with MAX alone, so the run-time specialised kernel or the VM evaluates the program as written"""
        q = Prog(self.arity, self.name + "+max")
        q.code, q.consts = list(self.code), list(self.consts)
        r = q.arity + len(q.code) - 1
        q.op("max", r, r)
        return q


def affine_prog(coefs, c):
    """c + a0 x0 + a1 x1 ..., written left to right"""
    p = Prog(len(coefs), "affine%d" % len(coefs))
    acc = p.k(c) if c is not None else None
    for i, a in enumerate(coefs):
        t = p.op("mul", p.k(a), i)
        acc = t if acc is None else p.op("add", acc, t)
    return p


def unary_prog(name):
    p = Prog(1, name)
    if name == "logistic":      # 1 / (1 + exp(-x)), the functor's own formula
        p.op("recip", p.op("add", p.k(1.0), p.op("exp", p.op("neg", 0))))
    else:
        p.op(name, 0)
    return p


def binary_prog(name):
    p = Prog(2, name)
    if name == "d_logistic":    # d * (s (1 - s)), s = 1 / (1 + exp(-x))
        s = p.op("recip", p.op("add", p.k(1.0), p.op("exp", p.op("neg", 1))))
        p.op("mul", 0, p.op("mul", s, p.op("sub", p.k(1.0), s)))
    elif name == "d_tanh":      # d * (1 - t t)
        t = p.op("tanh", 1)
        p.op("mul", 0, p.op("sub", p.k(1.0), p.op("mul", t, t)))
    elif name == "d_h1mh":      # d * (h (1 - h))
        p.op("mul", 0, p.op("mul", 1, p.op("sub", p.k(1.0), 1)))
    elif name == "d_1mh2":      # d * (1 - h h)
        p.op("mul", 0, p.op("sub", p.k(1.0), p.op("mul", 1, 1)))
    else:
        p.op(name, 0, 1)
    return p


def piecewise_prog(n):
    """the closure of the route tests that no functor matches: + - * abs max only, exact on small integers"""
    p = Prog(n, "piecewise%d" % n)
    y = 1 if n >= 2 else p.k(3.0)
    a = p.op("sub", p.op("abs", 0), y)
    b = p.op("mul", 0, y)
    r = p.op("add", p.op("max", a, b), y)
    for i in range(2, n):
        r = p.op("sub", r, p.op("abs", i))
    return p


FUNCTOR_UNARY = ("logistic", "exp", "log", "recip", "tanh", "sqrt")
FUNCTOR_BINARY = ("mul", "div", "d_logistic", "d_tanh")
PLANNER_BINARY = ("d_h1mh", "d_1mh2")       # functors only the lazy planner reaches; as closures they are specialised programs
EXACT_OPS = ("mul", "div", "recip", "sqrt", "neg", "abs")             # bit for bit numpy in the element type, on finite data
ZERO_SIGN_OPS = ("add", "sub", "mul", "div", "neg", "recip", "sqrt", "abs", "signum")


# ---- the rule of every opcode ----------------------------------------------------------------------------------------------------
# abs clears the sign bit (abs(-0.0) = +0.0, as numpy and the reference's `abs`); signum returns a zero or a NaN as it is
# (GHC's `signum`); max / min are the defaults of the reference's `Ord` -- `max x y = if x <= y then y else x`,
# `min x y = if x <= y then x else y` -- so with a NaN operand max gives its FIRST operand and min its SECOND, and
# max(+0, -0) = -0: neither numpy's `maximum` (NaN wins) nor C's fmax (NaN loses).
def _where(c, a, b):
    return np.where(c, a, b).astype(np.result_type(a, b))


RULES = {
    X_ADD: lambda a, b: a + b, X_SUB: lambda a, b: a - b, X_MUL: lambda a, b: a * b, X_DIV: lambda a, b: a / b,
    X_NEG: lambda a, b: -a, X_RECIP: lambda a, b: a.dtype.type(1) / a, X_EXP: lambda a, b: np.exp(a), X_LOG: lambda a, b: np.log(a),
    X_SQRT: lambda a, b: np.sqrt(a), X_ABS: lambda a, b: np.abs(a),
    X_SIGNUM: lambda a, b: _where(a > 0, a.dtype.type(1), _where(a < 0, a.dtype.type(-1), a)),
    X_SIN: lambda a, b: np.sin(a), X_COS: lambda a, b: np.cos(a), X_TANH: lambda a, b: np.tanh(a), X_POW: lambda a, b: np.power(a, b),
    X_MAX: lambda a, b: _where(a <= b, b, a), X_MIN: lambda a, b: _where(a <= b, a, b),
}


def ssa_eval(prog, xs, elem, work=np.longdouble):
    """the program on operands xs (arrays of one shape), every value held in `work`; constants pass through the element type
    first, as the device's do"""
    with np.errstate(all="ignore"):
        v = [np.asarray(x, dtype=elem).astype(work) for x in xs]
        shape = v[0].shape if v else ()
        last = {}
        for i, (op, a, b) in enumerate(prog.code):
            if op != X_CONST:
                last[a] = last[b] = i
        for i, (op, a, b) in enumerate(prog.code):
            if op == X_CONST:
                v.append(np.full(shape, np.asarray(prog.consts[a], dtype=elem).astype(work), dtype=work))
                continue
            v.append(np.asarray(RULES[op](v[a], v[b]), dtype=work))
            for o in (a, b):                 # (the 128 MiB cases: a value nobody reads again is dropped)
                if last[o] == i:
                    v[o] = None
        return v[-1]


def compare(got, prog, xs, elem, exact=False, zero_sign=False, fused=False):
    """per element: NaN where the reference is NaN, infinities with their sign, the sign of a zero (if asked), and finite
    values inside tol * max(|want|, 1) + 4 |numpy in the element type - want|; exact: bit for bit numpy in the element type on
    finite data.  Returns a description of the first failures, or None.

    An INTERMEDIATE value outside the element type's range (h (1 - h) at the largest finite h is -inf there and 1e77 in long
    double) makes the long-double evaluation describe another program: where its class and the class of numpy in the element
    type differ, the element type's IEEE arithmetic, step by step, is the reference.  fused: the evaluator is the affine
    functor, a chain of fma that does not round its products (0.5 inf - 2 max is inf there and inf - inf step by step): on
    those elements, and only there, the long-double class is accepted as well."""
    elem = np.dtype(elem).type
    ld = ssa_eval(prog, xs, elem)
    same = ssa_eval(prog, xs, elem, work=elem)
    got = np.asarray(got)
    if got.shape != ld.shape or got.dtype != np.dtype(elem):
        return "shape/dtype %s %s, expected %s %s" % (got.shape, got.dtype, ld.shape, np.dtype(elem))

    def against(want_ld):
        want = want_ld.astype(elem)
        bad = np.isnan(got) != np.isnan(want)
        inf = np.isinf(got) | np.isinf(want)
        bad |= inf & ~np.isnan(want) & ~np.isnan(got) & (got != want)
        fin = np.isfinite(got) & np.isfinite(want)
        band = TOL[elem] * np.maximum(np.abs(want_ld), 1) + 4 * np.where(np.isfinite(same), np.abs(same.astype(np.longdouble) - want_ld), 0)
        bad |= fin & ~(np.abs(got.astype(np.longdouble) - want_ld) <= band)
        if zero_sign:
            bad |= fin & (want == 0) & (got == 0) & (np.signbit(got) != np.signbit(want))
        return bad, want

    with np.errstate(all="ignore"):
        first = ld.astype(elem)
        off = (np.isnan(first) != np.isnan(same)) | (np.isinf(first) != np.isinf(same))
        bad, want = against(np.where(off, same.astype(np.longdouble), ld))
        if fused:
            bad = np.where(off, bad & against(ld)[0], bad)
        if exact:
            fs = np.isfinite(same) & np.all([np.isfinite(np.asarray(x, dtype=elem)) for x in xs], axis=0)
            bad |= fs & ((got != same) | (np.signbit(got) != np.signbit(same)))
    if not bad.any():
        return None
    idx = np.argwhere(bad)[:4]
    return "%s: %d of %d elements differ; first (index, inputs, want, got): %s" % (
        prog.name, int(bad.sum()), bad.size,
        [(tuple(int(j) for j in i), [float(np.asarray(x, dtype=elem)[tuple(i)]) for x in xs], float(want[tuple(i)]), float(got[tuple(i)])) for i in idx])


# ---- special values ---------------------------------------------------------------------------------------------------------------
def unary_values(dtype):
    """+-0, the least denormal and the least normal, +-1, +-inf, NaN; the overflow edges of exp in both types; the saturation
    ends of logistic and tanh; negative arguments for log and sqrt come with the signs"""
    fi = np.finfo(dtype)
    pos = [0.0, float(fi.smallest_subnormal), float(fi.tiny), 1.0, np.inf,
           88.7, 88.8, 103.9, 104.0, 709.7, 709.8, 745.0, 746.0, 110.0, 750.0, 1e-20, 20.0, 1e30, 0.5, 2.0]
    return np.array(pos + [-p for p in pos] + [np.nan], dtype=dtype)


def binary_values(dtype):
    fi = np.finfo(dtype)
    return np.array([0.0, -0.0, 1.0, -2.5, float(fi.smallest_subnormal), float(fi.max), np.inf, -np.inf, np.nan], dtype=dtype)


def binary_grid(dtype):
    v = binary_values(dtype)
    a, b = np.meshgrid(v, v, indexing="ij")
    return a.ravel().copy(), b.ravel().copy()


# ---- wide ranges ----------------------------------------------------------------------------------------------------------------
def wide_domain(name, dtype):
    """(lo, hi, both signs?) of |x|: the whole range on which the op's result is finite"""
    fi = np.finfo(dtype)
    big, tiny = float(fi.max), float(fi.smallest_subnormal)
    edge = 88.0 if np.dtype(dtype) == np.float32 else 709.0
    return {"exp": (tiny, edge, True), "logistic": (tiny, edge, True), "log": (tiny, big, False), "sqrt": (tiny, big, False),
            "recip": (4 * float(fi.tiny), 0.25 / float(fi.tiny), True), "tanh": (tiny, big, True), "neg": (tiny, big, True),
            "abs": (tiny, big, True), "mul": (float(fi.tiny) ** 0.5 * 4, big ** 0.5 / 4, True),
            "div": (float(fi.tiny) ** 0.5 * 4, big ** 0.5 / 4, True)}[name]


def wide_values(name, dtype, n=4096, seed=0):
    """n values log-uniform in magnitude over the op's domain, both signs where the op takes them"""
    lo, hi, signed = wide_domain(name, dtype)
    rng = np.random.default_rng(31 * sum(map(ord, name)) + np.dtype(dtype).itemsize + seed)
    x = np.exp(rng.uniform(np.log(lo), np.log(hi), n))
    if signed:
        x *= rng.choice((-1.0, 1.0), n)
    return np.clip(x, -hi, hi).astype(dtype)


# `c + a x` with |c| >> |a|: the three programs of the issue by hand -- (c, a, x) -- and a seeded sweep with |c| / |a| up to 1e16
# at |x| up to 1e12
AFFINE_BY_HAND = ((1.0, 1e-6, 1e6), (100.0, 0.001, 1e5), (1e8, 1e-8, 1e12))


def affine_sweep(count=24, seed=5):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        c = float(rng.choice((-1.0, 1.0)) * 10 ** rng.uniform(-8, 8))
        a = float(rng.choice((-1.0, 1.0)) * abs(c) / 10 ** rng.uniform(0, 16))
        out.append((c, a))
    return out


def affine_sweep_x(dtype, n=4096, seed=6):
    rng = np.random.default_rng(seed)
    return (np.exp(rng.uniform(np.log(1e-12), np.log(1e12), n)) * rng.choice((-1.0, 1.0), n)).astype(dtype)


# ---- random SSA programs ------------------------------------------------------------------------------------------------------------
N_RANDOM = 40
RANDOM_ELEMS = 1000


def _random_prog(rng, idx):
    """biased towards what stresses the slot allocator: an operand used twice in one instruction, values whose last use is
    far from their definition, many constants, a result that is an input or a constant, long chains through one slot"""
    arity = int(rng.integers(1, 9))
    n_instr = int(rng.choice((1, 2, 3, 5, 8, 13, 30, 60, 100, 200))) if rng.random() < 0.5 else int(rng.integers(1, 201))
    p = Prog(arity, "random%d" % idx)
    style = rng.choice(("mixed", "chain", "consts", "far"))
    held = []          # values kept for a use far away
    while len(p.code) < n_instr:
        nv = arity + len(p.code)
        left = n_instr - len(p.code)
        r = rng.random()

        def pick():
            if held and rng.random() < (0.5 if style == "far" else 0.15):
                return int(held[int(rng.integers(len(held)))])
            if style == "chain" and rng.random() < 0.8:
                return nv - 1
            if rng.random() < 0.3:
                return int(rng.integers(arity))
            return int(rng.integers(max(arity, nv - 6), nv)) if nv > arity else int(rng.integers(arity))
        if r < (0.45 if style == "consts" else 0.12):
            v = p.k(float(rng.choice((0.0, 1.0, -1.0, 0.5, 2.0, -0.25, 3.0, 1.5, -2.0, 0.125))))
        elif r < 0.25:
            a = pick()
            v = p.op(str(rng.choice(("add", "mul", "sub", "max", "min"))), a, a)       # ia == ib
        elif r < 0.45:
            v = p.op(str(rng.choice(("neg", "abs", "tanh", "sin", "cos", "signum"))), pick())
        elif r < 0.52 and left >= 3:     # guarded, as tools/expr_fuzz.py guards them: |b| + 0.5 below a quotient / under a root
            g = p.op("add", p.op("abs", pick()), p.k(0.5))
            v = p.op(str(rng.choice(("recip", "sqrt", "log"))), g) if rng.random() < 0.6 else p.op("div", pick(), g)
        elif r < 0.56 and left >= 3:
            v = p.op("exp", p.op("min", pick(), p.k(4.0)))
        else:
            v = p.op(str(rng.choice(("add", "sub", "mul", "max", "min", "add", "sub"))), pick(), pick())
        if rng.random() < 0.2:
            held.append(v)
        if len(held) > 12:
            held.pop(0)
    del p.code[n_instr:]                      # (a guarded group may run one or two past the count)
    p.consts = p.consts[:1 + max([a for op, a, b in p.code if op == X_CONST], default=-1)]
    last = rng.random()
    if last < 0.08:                           # the result is an input (`max x x` is x)
        i = int(rng.integers(arity))
        p.code[-1] = (X_MAX, i, i)
    elif last < 0.16:                         # the result is a constant
        p.consts.append(1.5)
        p.code[-1] = (X_CONST, len(p.consts) - 1, 0)
    return p


def random_inputs(prog, dtype, idx):
    rng = np.random.default_rng(1000 + idx)
    xs = [rng.uniform(-2, 2, RANDOM_ELEMS).astype(dtype) for _ in range(prog.arity)]
    xs[0][::7] = 0.0
    if prog.arity > 1:
        xs[1][3::11] = -0.0
    return xs


def program_is_kept(prog, dtype, idx):
    """the reference alone decides: finite on at least half the elements (an all-NaN program would pass vacuously), and numpy
    in the element type within an eighth of the tolerance of the long-double evaluation wherever both are finite -- a program
    numpy itself cannot evaluate that well tests conditioning, and these test the slot allocator"""
    if live_slots(prog) > slot_cap(dtype):     # (the VM refuses those: the slot-limit test has them)
        return False
    xs = random_inputs(prog, dtype, idx)
    want = ssa_eval(prog, xs, dtype)
    same = ssa_eval(prog, xs, dtype, work=np.dtype(dtype).type)
    fin = np.isfinite(want)
    if fin.sum() * 2 < fin.size or np.any(np.isfinite(want.astype(dtype)) != np.isfinite(same)):
        return False
    with np.errstate(all="ignore"):
        f2 = fin & np.isfinite(same)
        err = np.abs(same.astype(np.longdouble) - want)[f2]
        return bool(np.all(err <= TOL[np.dtype(dtype).type] / 8 * np.maximum(np.abs(want[f2]), 1)))


_PROGRAMS = {}


def random_programs(dtype):
    """N_RANDOM programs for the dtype, the same in every process (seeded; redrawn until kept)"""
    key = np.dtype(dtype).name
    if key not in _PROGRAMS:
        rng = np.random.default_rng(20240 + np.dtype(dtype).itemsize)
        out = []
        while len(out) < N_RANDOM:
            p = _random_prog(rng, len(out))
            if program_is_kept(p, dtype, len(out)):
                out.append(p)
        _PROGRAMS[key] = out
    return _PROGRAMS[key]


# ---- the VM's slot limit ------------------------------------------------------------------------------------------------------------
SLOT_BYTES = 96 * 4          # per thread: 96 fp32 / 48 fp64 values, 96 KiB of LDS a workgroup


def slot_cap(dtype):
    return SLOT_BYTES // np.dtype(dtype).itemsize


def slot_cases(dtype):
    """(k, runs?): the cap, one past it, and the first size past 64 KiB of LDS"""
    cap = slot_cap(dtype)
    return ((cap, True), (cap + 1, False), (cap * 2 // 3 + 1, True), (3, True))


def slots_prog(k):
    """exactly k values alive at once (the input's slot and k - 1 constants, each used once, at the end):
    x + 1 - 2 + 3 - 4 ...; every constant is distinct, so a slot handed out twice changes the sum"""
    p = Prog(1, "slots%d" % k)
    cs = [p.k(float(j + 1)) for j in range(k - 1)]
    acc = 0
    for j, c in enumerate(cs):
        acc = p.op("add" if j % 2 == 0 else "sub", acc, c)
    if not cs:
        p.op("add", 0, 0)
    return p


def live_slots(prog):
    """slots the allocator of csrc/expr.cpp needs: inputs keep theirs; a temporary's slot is free after its last use"""
    n, ar = len(prog.code), prog.arity
    last = {}
    for i, (op, a, b) in enumerate(prog.code):
        if op != X_CONST:
            last[a] = i
            last[b] = i
    last[ar + n - 1] = n
    slot, free, nxt = {i: i for i in range(ar)}, [], ar
    for i, (op, a, b) in enumerate(prog.code):
        if op != X_CONST:
            if a >= ar and last.get(a) == i:
                free.append(slot[a])
            if b >= ar and b != a and last.get(b) == i:
                free.append(slot[b])
        if free:
            slot[ar + i] = free.pop()
        else:
            slot[ar + i] = nxt
            nxt += 1
    return max(nxt, 1)
