"""Programs, formation rule and references for the row programs of csrc/rowprog.cpp (test infrastructure; imports no GPU
code).  tests/test_rowprog_cases.py checks the tables on the CPU, tests/test_gpu_rowprog.py runs them.

A program is a function `build(be, v)` over a backend `be` with the class methods' names (`liftT`, `gmul`, `sumT`, `scaleT`,
`sumRows`, `mapRows_const`, `konst`) and a dictionary `v` of operands: `z`, the root `W x` (recorded, never demanded), its
width `n`, and the externals the case asks for.  It returns the demanded values in order.  The same function records the graph on the device
(tests/test_gpu_rowprog.py), evaluates the float64 / long double reference (`Ref`) and runs row by row through the oracle's
`OTensor` (the CPU test).  `Ref` counts what a recording would hold -- member ops, constants, distinct externals -- and the
case states the same numbers by hand; `launches` restates `form_row_program_impl` (csrc/lazy_plan.cpp) on them.

Exact data: W and x are small integers, so z = W x is exact and differs from column to column with a period (7) no lane
stride shares; externals are small integers with periods 9 and 11; the closures of the exact programs use + - *, max, min, abs
and dyadic constants only.  Every value is then a multiple of 2^-6 far below 2^24 / 2^6, every partial sum of every reduction
is exactly representable in fp32 in any order (`Ref.exact_log`, checked on the CPU), and the device has to return the
reference bit for bit.

R_DACT is never recorded: the planner writes it (`rewrite_dlogistic`) over `d * logistic'(q)` / `d * tanh'(q)` when
`logistic q` / `tanh q` is in the plan, so its h is always the logistic or tanh of a plan node, never a free operand.  The exact
cases saturate it: q = 800 clamp(z, -1, 1) is -800, 0 or 800, where logistic gives 0, 1/2, 1 and tanh -1, 0, 1 bit for bit in
both element types (exp(800) = inf, exp(-800) = 0).  d h (1 - h) is then d / 4 at q = 0 and d (1 - h^2) is d: swapping the two
forms shows at every column with q = 0.

A closure of arity 0 cannot reach a program: `to_lift` refuses n = 0 (`use to_fill for constants`), and a recorded constant is
restated as a literal (R_CONST).  There is no such case."""
import numpy as np

DTYPES = (np.float32, np.float64)
DT_IDS = ("f32", "f64")
MAX_N, MAX_EXT, MAX_OUT, MIN_OPS = 1024, 4, 4, 2          # form_row_program_impl's admission
TOL = {np.float32: 1e-5, np.float64: 1e-12}               # the project's bound, per element against max(1, |ref|)
K = 3                                                     # the contraction's inner dimension


# ---- data ---------------------------------------------------------------------------------------------------------------------
def w_ints(N):
    """W [N, 3] in [-3, 3]: rows differ from their neighbours, period 7"""
    j, k = np.arange(N, dtype=np.int64)[:, None], np.arange(K, dtype=np.int64)[None, :]
    return ((j * (2 * k + 3) + 5 * k) % 7 - 3).astype(np.float64)


def x_ints(B):
    """x [B, 3]: the first entry in [1, 3] (no row of zeros), the others in [-2, 2] and [-3, 3]"""
    b = np.arange(B, dtype=np.int64)
    return np.stack([1 + b % 3, (2 * b) % 5 - 2, (3 * b) % 7 - 3], axis=1).astype(np.float64)


def ints(total, i):
    """small integers in [-4, 4], different at neighbouring positions, period 9"""
    return ((np.arange(total, dtype=np.int64) * (2 * i + 3) + 5 * i) % 9 - 4).astype(np.float64)


def ints11(total, i):
    """in [-5, 5], period 11"""
    return ((np.arange(total, dtype=np.int64) * (2 * i + 3) + 3 * i) % 11 - 5).astype(np.float64)


def probe_columns(N):
    """column 0, N - 1 and every multiple of 64, one less and one more, inside N"""
    cols = {0, N - 1}
    for m in range(64, N + 64, 64):
        cols.update(c for c in (m - 1, m, m + 1) if 0 <= c < N)
    return sorted(cols)


def probe_targets(B, N):
    """y [B, N]: probe column number i is hot in row i mod B -- a dropped or duplicated element of a dot product with y
    changes the row that holds its column, by that element"""
    y = np.zeros((max(B, 1), N))
    for i, c in enumerate(probe_columns(N)):
        y[i % max(B, 1), c] = 1.0
    return y


def external(kind, B, N, i):
    """the operand of one external: per-row vector [B, N], shared vector [N], per-row scalar [B], shared scalar []"""
    rows = max(B, 1)
    if kind == "vec_row":
        return ints(rows * N, i).reshape(rows, N)
    if kind == "vec_shared":
        return ints11(N, i)
    if kind == "sc_row":
        return ints(rows, i + 1)
    if kind == "sc_shared":
        return np.float64(-1.5 + i)
    if kind == "probe":
        return probe_targets(B, N)
    raise KeyError(kind)


# ---- closures -----------------------------------------------------------------------------------------------------------------
class NpMath:
    """the rule of every opcode on numpy arrays (tests/ewise_cases.py RULES: max / min are `Ord`'s defaults)"""
    @staticmethod
    def max(a, b):
        a, b = np.broadcast_arrays(np.asarray(a), np.asarray(b))
        return np.where(a <= b, b, a)

    @staticmethod
    def min(a, b):
        a, b = np.broadcast_arrays(np.asarray(a), np.asarray(b))
        return np.where(a <= b, a, b)

    abs = staticmethod(np.abs)
    exp = staticmethod(np.exp)
    log = staticmethod(np.log)
    tanh = staticmethod(np.tanh)

    @staticmethod
    def recip(a):
        return 1 / a


class Closure:
    """`fn(m, v)`: m the math namespace (NpMath here, symbolic values on the device), v the list of arguments"""

    def __init__(self, name, arity, fn):
        self.name, self.arity, self.fn = name, arity, fn

    def __call__(self, xs):
        with np.errstate(all="ignore"):
            return self.fn(NpMath, list(xs))


UN = Closure("un", 1, lambda m, v: m.max(v[0], 0.5 * v[0]) + 0.25)                       # never 0 on integers
BIN = Closure("bin", 2, lambda m, v: m.max(v[0], v[1]) - 0.5 * m.min(v[0], v[1]))
TERN = Closure("tern", 3, lambda m, v: v[0] * v[1] - m.abs(v[2]))
SAT = Closure("sat", 1, lambda m, v: 800.0 * m.max(-1.0, m.min(1.0, v[0])))
LOGISTIC = Closure("logistic", 1, lambda m, v: 1.0 / (1.0 + m.exp(-v[0])))
D_LOGISTIC = Closure("d_logistic", 2, lambda m, v: v[0] * (LOGISTIC.fn(m, v[1:]) * (1.0 - LOGISTIC.fn(m, v[1:]))))
TANH = Closure("tanh", 1, lambda m, v: m.tanh(v[0]))
D_TANH = Closure("d_tanh", 2, lambda m, v: v[0] * (1.0 - m.tanh(v[1]) * m.tanh(v[1])))
EXP = Closure("exp", 1, lambda m, v: m.exp(v[0]))
RECIP = Closure("recip", 1, lambda m, v: m.recip(v[0]))
LOG1 = Closure("log1", 1, lambda m, v: m.log(v[0]) + 1.0)
NEG_SQ = Closure("neg_sq", 1, lambda m, v: -(v[0] * v[0]))
EXACT_CLOSURES = (UN, BIN, TERN, SAT)


# ---- the reference backend ----------------------------------------------------------------------------------------------------
class V:
    """a value: `a` is [B, N] / [B] when batched, [N] / [] when shared by all rows"""
    __slots__ = ("a", "batched")

    def __init__(self, a, batched):
        self.a, self.batched = a, batched

    @property
    def rank(self):
        return self.a.ndim - (1 if self.batched else 0)


class Ref:
    """the class methods on numpy arrays in `work` (float64, or long double for the fp64 device), all rows at once; counts
    member ops, constants and distinct externals, and keeps what `exact_log` needs"""

    def __init__(self, work=np.float64):
        self.work = work
        self.n_ops = self.n_consts = 0
        self.externals = []          # ids of the leaves the ops have read
        self.values = []             # every value made
        self.reductions = []         # the terms of every row sum / dot product

    def leaf(self, a, batched):
        return V(np.asarray(a, dtype=self.work), batched)

    def _made(self, v, xs, op=True):
        self.n_ops += 1 if op else 0
        for x in xs:
            if getattr(x, "_leaf", False) and id(x) not in self.externals:
                self.externals.append(id(x))
        self.values.append(v.a)
        return v

    @staticmethod
    def _together(xs):
        batched = any(x.batched for x in xs)
        return [x.a if (x.batched or not batched) else x.a[None] for x in xs], batched

    def liftT(self, f, xs):
        assert len(xs) == f.arity and len({x.rank for x in xs}) == 1
        arrs, batched = self._together(xs)
        arrs = np.broadcast_arrays(*arrs)
        return self._made(V(np.asarray(f(arrs), dtype=self.work), batched), xs)

    def sumT(self, xs, shape):
        arrs, batched = self._together(xs)
        acc = arrs[0]
        with np.errstate(all="ignore"):
            for a in arrs[1:]:
                acc = acc + a                   # a left fold, like sum'
        return self._made(V(np.asarray(acc, dtype=self.work), batched), xs)

    def scaleT(self, alpha, x):
        with np.errstate(all="ignore"):
            return self._made(V(self.work(alpha) * x.a, x.batched), [x])

    def sumRows(self, x):
        assert x.rank == 1
        self.reductions.append(x.a)
        with np.errstate(all="ignore"):
            return self._made(V(x.a.sum(axis=-1), x.batched), [x])

    def mapRows_const(self, len_n, row, like):
        assert len_n == 1 and row.rank == 0 and like.rank == 1
        n = like.a.shape[-1]
        return self._made(V(np.repeat(row.a[..., None], n, axis=-1), row.batched), [row])

    def konst(self, shape, c):
        self.n_consts += 1
        return self._made(V(np.full(tuple(shape), c, dtype=self.work), False), [], op=False)

    def gmul(self, lm, lo, ln, x, y):
        (a, b), batched = self._together([x, y]) if x.rank == y.rank else ((x.a, y.a), x.batched or y.batched)
        with np.errstate(all="ignore"):
            if (lm, lo, ln) == (0, 1, 0):            # a dot product of two vectors
                a, b = np.broadcast_arrays(a, b)
                self.reductions.append(a * b)
                return self._made(V((a * b).sum(axis=-1), batched), [x, y])
            if (lm, lo, ln) == (0, 0, 1):            # scalar x vector
                assert x.rank == 0 and y.rank == 1
                s = x.a[..., None] if x.batched else x.a
                return self._made(V(np.asarray(s * y.a, dtype=self.work), batched), [x, y])
            if (lm, lo, ln) == (0, 0, 0):
                return self._made(V(np.asarray(x.a * y.a, dtype=self.work), batched), [x, y])
        raise NotImplementedError((lm, lo, ln))

    def exact_log(self):
        """None if every value made is a multiple of 2^-6 that fp32 holds and every reduction's terms sum, in absolute value,
        below 2^24 units of 2^-6 (then every partial sum, in any order, is exact in fp32); else what is not"""
        for a in self.values:
            a = np.asarray(a, dtype=np.float64)
            if not np.isfinite(a).all() or not np.array_equal(a * 64, np.round(a * 64)) or not np.array_equal(a.astype(np.float32), a):
                return "a value is no fp32 multiple of 2^-6"
        for t in self.reductions:
            if (np.abs(np.asarray(t, dtype=np.float64)) * 64).sum(axis=-1).max() >= 2.0 ** 24:
                return "a reduction's partial sums can leave fp32's integers"
        return None


def root_data(case, B, N):
    """(W [N, 3], x [B, 3] or [3]) of a case: integers, or the constant rows of the dead-lane cases"""
    rows = max(B, 1)
    if case.get("root") == "zeros":
        W, x = w_ints(N), np.zeros((rows, K))
    elif case.get("root") == "ones":
        W, x = np.tile([1.0, 2.0, -3.0], (N, 1)), np.tile([1.0, 0.0, 0.0], (rows, 1))
    else:
        W, x = w_ints(N), x_ints(rows)
    return W, (x if B > 0 else x[0])


def operands(case, B, N):
    """name -> (kind, numpy array) of the case's externals, in the order given"""
    return {name: (kind, external(kind, B, N, i)) for i, (name, kind) in enumerate(case["ext"])}


def peer_data(B, N):
    """the second contraction W' s of the peer cases: W' [N, 3] = W reversed along k, s [B, 3] small integers"""
    return w_ints(N)[:, ::-1].copy(), ints(max(B, 1) * K, 7).reshape(max(B, 1), K)


def dyadic(total):
    """k / 8 in [0, 1]"""
    return (np.arange(total, dtype=np.int64) * 5 % 9) / 8.0


def reference(case, B, N, work=np.float64, x=None, W=None):
    """(demanded values as numpy arrays in `work`, the Ref that made them); B = 0: the unbatched root"""
    be = Ref(work)
    W0, x0 = root_data(case, B, N)
    W = np.asarray(W0 if W is None else W, dtype=work)
    x = np.asarray(x0 if x is None else x, dtype=work)
    v = {"n": N}
    with np.errstate(all="ignore"):
        from nonfinite_ref import contract
        z = x @ W.T if np.isfinite(x).all() else contract(np.atleast_2d(x), W.T).reshape(x.shape[:-1] + (N,))
    v["z"] = V(np.asarray(z, dtype=work), B > 0)
    for name, (kind, a) in operands(case, B, N).items():
        per_row = kind in ("vec_row", "sc_row", "probe")
        a = np.asarray(a, dtype=work)
        leaf = V(a if (B > 0 or not per_row) else a[0], per_row and B > 0)
        v[name] = _Leaf(leaf)
    if case.get("peer"):
        Wp, s = peer_data(B, N)
        p = np.asarray(s if B > 0 else s[0], dtype=work) @ np.asarray(Wp, dtype=work).T
        v["p"] = _Leaf(V(p, B > 0))
    outs = case["build"](be, v)
    return [o.a for o in outs], be


class _Leaf(V):
    __slots__ = ("_leaf",)

    def __init__(self, v):
        super().__init__(v.a, v.batched)
        self._leaf = True


# ---- the programs -------------------------------------------------------------------------------------------------------------
# Each program's first op is one the contraction's own epilogue does not take (a piecewise closure, a row sum, a closure of two
# operands), or z has a second consumer.
def p_lift_vec(be, v):                # R_LIFT on vectors: unary, binary
    t = be.liftT(UN, [v["z"]])
    return [be.liftT(BIN, [t, v["a"]])]


def p_lift_vec3(be, v):               # R_LIFT on vectors: ternary, mixing a per-row and a shared operand
    t = be.liftT(TERN, [v["z"], v["a"], v["u"]])
    return [be.liftT(UN, [t])]


def p_lift_scalar(be, v):             # R_LIFT on per-row scalars: unary, binary, ternary
    s = be.sumRows(v["z"])
    t = be.liftT(UN, [s])
    return [be.liftT(BIN, [t, v["r"]]), be.liftT(TERN, [s, v["c"], t])]


def _dact(act, d_act):
    def build(be, v):
        q = be.liftT(SAT, [v["z"]])
        h = be.liftT(act, [q])
        return [be.liftT(d_act, [v["a"], q]), h]     # (the planner rewrites the first into R_DACT over h)
    return build


def p_sum(be, v):                     # R_SUM: 2-ary and 3-ary, a vector with a shared vector
    t = be.liftT(UN, [v["z"]])
    n = v["n"]
    return [be.sumT([t, v["u"]], (n,)), be.sumT([v["u"], t, v["z"]], (n,))]


def p_scale(be, v):
    return [be.scaleT(-1.5, be.liftT(UN, [v["z"]]))]


def p_mul(be, v):                     # R_MUL: scalar x vector, scalar x scalar
    s = be.sumRows(v["z"])
    return [be.gmul(0, 0, 1, s, v["z"]), be.gmul(0, 0, 0, s, v["r"])]


def p_sum_rows(be, v):
    return [be.sumRows(be.liftT(UN, [v["z"]]))]


def p_dot(be, v):
    return [be.gmul(0, 1, 0, be.liftT(UN, [v["z"]]), v["a"])]


def p_map_rows(be, v):
    return [be.mapRows_const(1, be.sumRows(v["z"]), v["u"])]


def p_const(be, v):                   # R_CONST: a vector and a scalar
    n = v["n"]
    t = be.liftT(BIN, [v["z"], be.konst((n,), 2.5)])
    return [t, be.liftT(BIN, [be.sumRows(t), be.konst((), -3.0)])]


def p_width(be, v):                   # the exact program of the width table: a row sum, a dot product, a vector output
    t = be.liftT(UN, [v["z"]])
    s = be.sumRows(t)
    return [s, be.gmul(0, 1, 0, t, v["y"]), be.gmul(0, 0, 1, s, t)]


def _normalised(f):                   # e = f z; s = sumRows e; p = (1 / s) e
    def build(be, v):
        e = be.liftT(f, [v["z"]])
        s = be.sumRows(e)
        return [s, be.gmul(0, 0, 1, be.liftT(RECIP, [s]), e)]
    return build


def _chain(be, v, first):
    """a vector through four operand kinds: per-row vector (twice), shared vector, per-row scalar, shared scalar"""
    t = be.liftT(TERN, [first, v["u"], v["a"]])
    s = be.sumRows(t)
    s2 = be.liftT(BIN, [s, v["r"]])
    return t, s, s2, be.liftT(BIN, [s2, v["c"]])


def p_ext4(be, v):                    # 4 externals; `a` is recorded twice
    t, _, _, s3 = _chain(be, v, be.liftT(BIN, [v["z"], v["a"]]))
    return [t, s3]


def p_ext5(be, v):                    # one more: no program
    t, _, _, s3 = _chain(be, v, be.liftT(BIN, [be.liftT(BIN, [v["z"], v["b"]]), v["a"]]))
    return [t, s3]


def p_peer(be, v):                    # the output of a second contraction of the same plan, read like an existing tensor
    t = be.liftT(BIN, [v["z"], v["p"]])
    return [be.liftT(UN, [t]), be.sumRows(t)]


def p_peer5(be, v):                   # 4 externals and a peer: the branch that reads the peer stays out, the rest is a program
    t, _, _, s3 = _chain(be, v, be.liftT(BIN, [v["z"], v["a"]]))
    return [t, s3, be.liftT(BIN, [v["z"], v["p"]])]


def p_out4(be, v):                    # 4 outputs, vectors and scalars
    return list(_chain(be, v, be.liftT(BIN, [v["z"], v["a"]])))


def p_out5(be, v):
    t, s, s2, s3 = _chain(be, v, be.liftT(BIN, [v["z"], v["a"]]))
    return [t, s, s2, s3, be.liftT(UN, [t])]


def p_inf(be, v):                     # an infinite R_SCALE factor and an infinite R_CONST: jit_literal's special branch
    t = be.liftT(UN, [v["z"]])
    n = v["n"]
    return [be.scaleT(np.inf, t), be.liftT(BIN, [t, be.konst((n,), -np.inf)])]


def p_nonfinite(be, v):               # the exact program of the non-finite table: + - * only (no comparison sees a NaN)
    t = be.liftT(NEG_SQ, [v["z"]])
    s = be.sumRows(t)
    return [s, be.gmul(0, 1, 0, t, v["a"]), be.sumT([t, v["u"]], (v["n"],))]


def composite_reference(z, y, work=np.float64):
    """softmax >>> scale 0.5 >>> squaredError against y, and its cotangent: (loss [B], dz [B, N]) in closed form.
    p = exp z / sum exp z (as recorded: no maximum is subtracted); o = p / 2; loss = sum (y - o)^2;
    dz_j = p_j (g_j - sum_i g_i p_i) with g = dloss/dp = -(y - o)"""
    z, y = np.asarray(z, dtype=work), np.asarray(y, dtype=work)
    e = np.exp(z)
    p = e / e.sum(axis=-1, keepdims=True)
    r = y - p / 2
    g = -r
    return (r * r).sum(axis=-1), p * (g - (g * p).sum(axis=-1, keepdims=True))


# The head as the host mirror records it (value, and cotangent of z alone): 19 ops -- exp, sumRows, recip, the outer product,
# two scales (softmax's own 1 and the 0.5), negate-and-add, the dot; then seed * r twice, their sum, the scales back, and the
# cotangent of softmax: a dot, a closure of two scalars, mapRows, a product, a sum, a closure of two vectors -- and one
# constant, the seed of gradTOp.  Without a program the product `seed * r` is a GEMM group again and takes the three ops behind
# it (the sum as its C operand, the two scales as alpha / beta) into its epilogue, as form_gemm_group does for any contraction.
COMPOSITE_OPS, COMPOSITE_CONSTS, COMPOSITE_EPILOGUE = 19, 1, 3


def _case(id, build, ext, ops, consts=0, outs=1, **kw):
    n_ext = len(ext) - len(kw.get("like_only", ())) + (1 if kw.get("peer") else 0)       # (`like` gives mapRows a shape, no operand)
    return dict(id=id, build=build, ext=tuple(ext), n_ops=ops, n_consts=consts, n_outs=outs, n_ext=n_ext, **kw)


A, U, R, C, B2 = ("a", "vec_row"), ("u", "vec_shared"), ("r", "sc_row"), ("c", "sc_shared"), ("b", "vec_row")

# a. one program per RowOp, as small as formation allows (the root and two ops)
OP_CASES = [
    _case("lift-vec", p_lift_vec, [A], 2),
    _case("lift-vec3", p_lift_vec3, [A, U], 2),
    _case("lift-scalar", p_lift_scalar, [R, C], 4, outs=2),
    _case("dact-logistic", _dact(LOGISTIC, D_LOGISTIC), [A], 3, outs=2, dact=True),
    _case("dact-tanh", _dact(TANH, D_TANH), [A], 3, outs=2, dact=True),
    _case("sum", p_sum, [U], 3, outs=2),
    _case("scale", p_scale, [], 2),
    _case("mul", p_mul, [R], 3, outs=2),
    _case("sum-rows", p_sum_rows, [], 2),
    _case("dot", p_dot, [A], 2),
    _case("map-rows", p_map_rows, [U], 2, like_only=("u",)),
    _case("const", p_const, [], 3, consts=2, outs=2),
]
WIDTH_CASE = _case("width", p_width, [("y", "probe")], 4, outs=3)
# c. dead lanes: z = 0 under exp, z = 1 under recip and log + 1 -- the lanes past N hold exp 0 = 1, 1 / 0 = inf, log 0 = -inf
DEAD_CASES = [
    _case("dead-exp", _normalised(EXP), [], 4, outs=2, root="zeros"),
    _case("dead-recip", _normalised(RECIP), [], 4, outs=2, root="ones"),
    _case("dead-log", _normalised(LOG1), [], 4, outs=2, root="ones"),
]
# d. external operands and the limits
EXT_CASES = [
    _case("ext-4", p_ext4, [A, U, R, C], 5, outs=2),
    _case("ext-5", p_ext5, [A, U, R, C, B2], 6, outs=2),
    _case("peer", p_peer, [], 3, outs=2, peer=True),
    _case("peer-5", p_peer5, [A, U, R, C], 6, outs=3, peer=True, retry_ops=5, retry_outs=2),
    _case("out-4", p_out4, [A, U, R, C], 5, outs=4),
    _case("out-5", p_out5, [A, U, R, C], 6, outs=5),
]
INF_CASE = _case("inf-literals", p_inf, [], 3, consts=1, outs=2)
NONFINITE_CASE = _case("nonfinite", p_nonfinite, [A, U], 4, outs=3)
ALL_CASES = OP_CASES + [WIDTH_CASE] + DEAD_CASES + EXT_CASES + [INF_CASE, NONFINITE_CASE]

OP_N, OP_B = 65, 5                                   # EPL = 2, one live lane in the second trip, one live wave in the last workgroup
WIDTHS = (1, 17, 63, 64, 65, 127, 128, 129, 784, 1000, 1023, 1024, 1025)
WIDTHS_F64 = (65, 1000, 1024, 1025)                  # (a build per width and type: the fp64 side keeps the edges of the limit)
BATCHES = (1, 3, 4, 5, 130)                          # all of them at N = 65, B = 5 elsewhere; 0 = the unbatched root, at N = 65
DEAD_WIDTHS = (65, 1000)
INEXACT_WIDTHS = (65, 784, 1024)


def widths(dt):
    return WIDTHS if np.dtype(dt) == np.float32 else WIDTHS_F64


def width_shapes(dt):
    """(N, B) of the width table"""
    return [(N, OP_B) for N in widths(dt)] + [(OP_N, B) for B in BATCHES if B != OP_B] + [(OP_N, 0)]


# ---- the formation rule ---------------------------------------------------------------------------------------------------------
def forms(N, n_ext, n_outs, n_ops):
    """form_row_program_impl: a rank-1 root of 1 .. 1024 elements, at most 4 distinct existing operands, 1 .. 4 values the
    rest of the graph needs, at least two member ops (the root and a single op is one launch already)"""
    return 1 <= N <= MAX_N and n_ext <= MAX_EXT and 1 <= n_outs <= MAX_OUT and n_ops >= MIN_OPS


def launches(case, N, rowprog_on=True):
    """launches BEHIND the contractions' own: 1 if a program forms and runs, else one per member op and per constant.  With
    more than 4 operands, peers among them, the planner tries again without peers: the ops that read one stay out (one launch
    each) and the rest may form"""
    every = case["n_ops"] + case["n_consts"]
    if not rowprog_on:
        return every
    if forms(N, case["n_ext"], case["n_outs"], case["n_ops"]):
        return 1
    if case.get("peer") and case["n_ext"] > MAX_EXT and forms(N, case["n_ext"] - 1, case["retry_outs"], case["retry_ops"]):
        return 1 + (case["n_ops"] - case["retry_ops"])
    return every


def formed(case, N):
    return launches(case, N) < case["n_ops"] + case["n_consts"]


def elided(case, N, rowprog_on=True):
    """what `to_lazy_stats`' elided counter gains: the members of a program that ran, less its outputs"""
    if not (rowprog_on and formed(case, N)):
        return 0
    whole = forms(N, case["n_ext"], case["n_outs"], case["n_ops"])
    return (case["n_ops"] + case["n_consts"] - case["n_outs"]) if whole else case["retry_ops"] - case["retry_outs"]


def composite_launches(N, rowprog_on=True):
    """behind the contraction: a program is planned at N <= 1024 -- 1 launch, or its 20 members one by one when programs are
    off; none is planned beyond -- 20 less the 3 ops in the epilogue of `seed * r`"""
    if forms(N, 1, 2, COMPOSITE_OPS):
        return 1 if rowprog_on else COMPOSITE_OPS + COMPOSITE_CONSTS
    return COMPOSITE_OPS + COMPOSITE_CONSTS - COMPOSITE_EPILOGUE


def composite_elided(N, rowprog_on=True):
    if forms(N, 1, 2, COMPOSITE_OPS):
        return COMPOSITE_OPS + COMPOSITE_CONSTS - 2 if rowprog_on else 0
    return COMPOSITE_EPILOGUE


# ---- non-finite inputs --------------------------------------------------------------------------------------------------------
def poisoned_x(B):
    """x_ints with NaN, +inf, -inf at chosen (row, k): rows 1, 2 and 4 of 5 are poisoned, 0 and 3 are not"""
    x = x_ints(B)
    x[1, 0], x[2, 1], x[4, 2] = np.nan, np.inf, -np.inf
    return x, (0, 3)


def same_with_nan(got, want):
    """element for element, NaN where the reference has NaN (tests/nonfinite_ref.py's convention)"""
    got, want = np.asarray(got), np.asarray(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[~np.isnan(want)], want[~np.isnan(want)])


def within(got, want, tol):
    """|got - ref| <= tol max(1, |ref|) per element; returns (ok, the largest |got - ref| / max(1, |ref|))"""
    got, want = np.asarray(got, dtype=np.longdouble), np.asarray(want, dtype=np.longdouble)
    err = np.abs(got - want) / np.maximum(1, np.abs(want))
    worst = float(err.max()) if err.size else 0.0
    return bool(got.shape == want.shape and np.isfinite(got).all() and worst <= tol), worst
