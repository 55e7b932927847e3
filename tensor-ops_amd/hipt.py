"""`class Tensor` (src/TensorOps/Types.hs:52-109) over device handles, via the C ABI.

Harness-side plumbing only: every method is one or two C-ABI calls, named as in
the reference so parity tests read like the reference's own code.  Closures
passed to `liftT` are reified the way a Haskell shim would do it: they are
applied to symbolic scalars (`Sym`) that record an SSA program, which is
compiled once by `to_expr_compile` and cached.
"""
import ctypes as C
import itertools
import os
import sys

import numpy as np

from . import capi
from .capi import check, dims_arr, lib

# opcodes (include/tensorops_hip.h)
(X_CONST, X_ADD, X_SUB, X_MUL, X_DIV, X_NEG, X_RECIP, X_EXP, X_LOG, X_SQRT, X_ABS, X_SIGNUM, X_SIN,
 X_COS, X_TANH, X_POW, X_MAX, X_MIN) = range(18)
_UNARY = {"exp": X_EXP, "log": X_LOG, "sqrt": X_SQRT, "sin": X_SIN, "cos": X_COS, "tanh": X_TANH,
          "abs_": X_ABS, "abs": X_ABS, "recip": X_RECIP, "signum": X_SIGNUM}


_DL_SENTINEL = bool(os.environ.get("TOPS_DL_SENTINEL"))


def _report_unwritten(raw, out):
    """TOPS_DL_SENTINEL=1 (tools/stress_suite.py): the destination of every download is filled with 0xFFA5C3E1 words first
    (a NaN no kernel here produces); words that still hold it after to_download returned were never written."""
    left = np.flatnonzero(raw == 0xFFA5C3E1)
    if not len(left):
        return
    cuts = np.flatnonzero(np.diff(left) > 16) + 1
    runs = [(int(r[0]) * 4, int(r[-1] - r[0] + 1) * 4) for r in np.split(left, cuts)[:24]]
    msg = ("DIAG download left %d of %d words UNWRITTEN (pid %d, shape %s %s, dst %#x, dst mod 4096 = %d, staging %s): runs (byte offset, bytes) %s"
           % (len(left), raw.size, os.getpid(), out.shape, out.dtype, out.ctypes.data, out.ctypes.data % 4096,
              os.environ.get("TOPS_PINNED_STAGING", "on"), runs))
    print(msg, file=sys.stderr, flush=True)
    d = os.environ.get("TOPS_MISMATCH_DIR")
    if d:
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, "unwritten_%d.txt" % os.getpid()), "a") as f:
            f.write(msg + "\n")


class _Tape:
    def __init__(self, arity):
        self.arity = arity
        self.code = []
        self.consts = []
        self.cse = {}

    def emit(self, op, a, b=0):
        key = (op, a, b)
        if key in self.cse:
            return self.cse[key]
        self.code.append(key)
        v = self.arity + len(self.code) - 1
        self.cse[key] = v
        return v

    def const(self, c):
        c = float(c)
        key = ("c", c.hex())
        if key in self.cse:
            return self.cse[key]
        self.consts.append(c)
        self.code.append((X_CONST, len(self.consts) - 1, 0))
        v = self.arity + len(self.code) - 1
        self.cse[key] = v
        return v


class Sym:
    """Symbolic element: what `ElemT HipT` is while a closure is being reified."""
    __array_ufunc__ = None

    def __init__(self, tape, v):
        self.tape = tape
        self.v = v

    def _lift(self, o):
        if isinstance(o, Sym):
            return o
        return Sym(self.tape, self.tape.const(o))

    def _bin(self, op, o, swap=False):
        o = self._lift(o)
        a, b = (o.v, self.v) if swap else (self.v, o.v)
        return Sym(self.tape, self.tape.emit(op, a, b))

    def __add__(self, o): return self._bin(X_ADD, o)
    def __radd__(self, o): return self._bin(X_ADD, o, True)
    def __sub__(self, o): return self._bin(X_SUB, o)
    def __rsub__(self, o): return self._bin(X_SUB, o, True)
    def __mul__(self, o): return self._bin(X_MUL, o)
    def __rmul__(self, o): return self._bin(X_MUL, o, True)
    def __truediv__(self, o): return self._bin(X_DIV, o)
    def __rtruediv__(self, o): return self._bin(X_DIV, o, True)
    def __pow__(self, o): return self._bin(X_POW, o)
    def __neg__(self): return Sym(self.tape, self.tape.emit(X_NEG, self.v, self.v))
    def __abs__(self): return self.__tops_unary__("abs")

    def __tops_unary__(self, name):
        return Sym(self.tape, self.tape.emit(_UNARY[name], self.v, self.v))

    # seeds for forward-mode AD over symbolic values (oracle.ad / host mirror)
    def one_like(self): return 1.0
    def zero_like(self): return 0.0


def _sym_unary(name):
    def f(x):
        return x.__tops_unary__(name)
    return f


exp, log, sqrt, sin, cos, tanh, recip = (_sym_unary(n) for n in
                                         ("exp", "log", "sqrt", "sin", "cos", "tanh", "recip"))


def maximum(a, b):
    """`max a b` on symbolic values (either may be a number)."""
    s = a if isinstance(a, Sym) else b
    return s._lift(a)._bin(X_MAX, b)


def minimum(a, b):
    s = a if isinstance(a, Sym) else b
    return s._lift(a)._bin(X_MIN, b)


def logistic_closure(v):
    """`logistic x = 1 / (1 + exp (-x))` (src/TensorOps/Learn/NeuralNet.hs:42-44) on symbolic input."""
    return 1.0 / (1.0 + exp(-v[0]))


class Expr:
    """A compiled elementwise expression handle."""

    def __init__(self, arity, code, consts):
        flat = (C.c_int32 * max(3 * len(code), 1))(*[int(x) for ins in code for x in ins])
        cs = (C.c_double * max(len(consts), 1))(*consts)
        h = capi.c_expr()
        check(lib().to_expr_compile(arity, len(code), flat, len(consts), cs, C.byref(h)))
        self.h = h
        self.arity = arity

    @property
    def kind(self):
        k = C.c_int()
        check(lib().to_expr_kind(self.h, C.byref(k)))
        return k.value

    def __del__(self):
        try:
            if self.h:
                lib().to_expr_release(self.h)
        except Exception:
            pass


def reify(f, n):
    """Apply `f :: [a] -> a` to n symbolic inputs and compile the recorded program."""
    tape = _Tape(n)
    r = f([Sym(tape, i) for i in range(n)])
    if not isinstance(r, Sym):
        r = Sym(tape, tape.const(r))
    if r.v != tape.arity + len(tape.code) - 1:
        # make the result the last value: result * 1 would change rounding, so re-emit a copy
        # through `x + 0` only when the result is an input or an earlier value
        z = tape.const(0.0)
        tape.code.append((X_ADD, r.v, z))
    return Expr(n, tape.code, tape.consts)


class DT:
    """Device tensor: owns one reference to a `to_tensor` handle."""
    __slots__ = ("h",)
    __array_ufunc__ = None

    def __init__(self, h):
        self.h = h

    def __del__(self):
        try:
            if self.h:
                lib().to_release(self.h)
        except Exception:
            pass

    def _shape(self):
        rank = C.c_int()
        dims = (C.c_int64 * 8)()
        batch = C.c_int64()
        check(lib().to_shape(self.h, C.byref(rank), dims, C.byref(batch)))
        return tuple(dims[i] for i in range(rank.value)), batch.value

    @property
    def shape(self):
        return self._shape()[0]

    @property
    def batch(self):
        return self._shape()[1]

    @property
    def ptr(self):
        p = C.c_void_p()
        check(lib().to_data_ptr(self.h, C.byref(p)))
        return p.value

    def numpy(self):
        """Download: logical row-major; shape (B, *ns) when batched."""
        shape, batch = self._shape()
        full = ((batch,) if batch > 0 else ()) + shape
        out = np.empty(full, dtype=self.dtype)
        sentinel = _DL_SENTINEL and out.nbytes >= 4
        if sentinel:   # (harness diagnostics: does the download write every byte of its destination?)
            raw = out.reshape(-1).view(np.uint32)
            raw[:] = 0xFFA5C3E1
        check(lib().to_download(self.h, out.ctypes.data_as(C.c_void_p), out.nbytes))
        if sentinel:
            _report_unwritten(raw, out)
        return out

    @property
    def dtype(self):
        dt = C.c_int()
        check(lib().to_dtype(self.h, C.byref(dt)))
        return np.dtype(np.float64 if dt.value == capi.TO_F64 else np.float32)


def _out():
    return capi.c_tensor()


def _arr(ts):
    return (capi.c_tensor * max(len(ts), 1))(*[t.h for t in ts])


class HipT:
    """The backend dictionary (`instance Tensor HipT`); `ElemT` is float32 (default) or float64."""

    def __init__(self, device=0, dtype=np.float32):
        check(lib().to_init(device))
        self._exprs = {}
        self.dtype = np.dtype(dtype)
        if self.dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
            raise ValueError("HipT: ElemT must be float32 or float64")
        self.to_dtype = capi.TO_F64 if self.dtype == np.dtype(np.float64) else capi.TO_F32

    # -- host <-> device ----------------------------------------------------------
    def put(self, x, batched=False):
        """`fromList`/`generateA`: build on the host, upload once."""
        x = np.asarray(x, dtype=self.dtype, order="C")
        batch = 0
        shape = x.shape
        if batched:
            batch, shape = x.shape[0], x.shape[1:]
        d, r = dims_arr(shape)
        h = _out()
        check(lib().to_from_host(self.to_dtype, r, d, batch, x.ctypes.data_as(C.c_void_p), C.byref(h)))
        return DT(h)

    def from_list(self, shape, xs):
        n = int(np.prod(shape)) if len(shape) else 1
        xs = list(xs)
        if len(xs) < n:
            return None
        return self.put(np.array(xs[:n], dtype=self.dtype).reshape(tuple(shape)))

    def generate(self, shape, f):
        out = np.empty(tuple(shape), dtype=self.dtype)
        for i in itertools.product(*[range(d) for d in shape]):
            out[i] = f(i)
        return self.put(out)

    def konst(self, shape, x):
        d, r = dims_arr(shape)
        h = _out()
        check(lib().to_fill(self.to_dtype, r, d, 0, float(x), C.byref(h)))
        return DT(h)

    def genRand(self, shape, dist, a, b, seed, batch=0):
        d, r = dims_arr(shape)
        h = _out()
        check(lib().to_rand(self.to_dtype, r, d, batch, {"uniform": 0, "normal": 1, "exponential": 2, "cauchy": 3, "laplace": 4}[dist], a, b, seed,
                            C.byref(h)))
        return DT(h)

    # -- class methods ------------------------------------------------------------------
    def expr(self, f, n, key=None):
        key = key if key is not None else (f, n)
        e = self._exprs.get(key)
        if e is None:
            e = reify(f, n)
            self._exprs[key] = e
        return e

    def liftT(self, f, xs, key=None):
        e = f if isinstance(f, Expr) else self.expr(f, len(xs), key)
        h = _out()
        check(lib().to_lift(e.h, len(xs), _arr(xs), C.byref(h)))
        return DT(h)

    def gmul(self, len_m, len_o, len_n, x, y):
        h = _out()
        check(lib().to_gmul(len_m, len_o, len_n, x.h, y.h, C.byref(h)))
        return DT(h)

    # TT.inner / outer / outerV / dot / matVec / vecMat / matMat (Tensor.hs:132-185): gmul with |os| = 1 or 0
    def inner(self, len_m, len_n, x, y): return self.gmul(len_m, 1, len_n, x, y)
    def outer(self, len_m, len_n, x, y): return self.gmul(len_m, 0, len_n, x, y)
    def outerV(self, x, y): return self.gmul(1, 0, 1, x, y)
    def dot(self, x, y): return self.gmul(0, 1, 0, x, y)
    def matVec(self, a, x): return self.gmul(1, 1, 0, a, x)
    def vecMat(self, x, a): return self.gmul(0, 1, 1, x, a)
    def matMat(self, a, b): return self.gmul(1, 1, 1, a, b)

    # TT.toList / elems / unScalar / toRows / rows (Tensor.hs:193-273): one download, host traversal
    def toList(self, x): return [float(v) for v in x.numpy().ravel()]
    elems = toList
    def unScalar(self, x): return float(x.numpy())
    def toRows(self, x): return [self.slice(x, (i,)) for i in range(x.shape[0])]
    def rows(self, rs): return self.stack((len(rs),), rs)

    def gmul_batch_sum(self, len_m, len_o, len_n, x, y):
        h = _out()
        check(lib().to_gmul_batch_sum(len_m, len_o, len_n, x.h, y.h, C.byref(h)))
        return DT(h)

    def sumT(self, xs, shape):
        if len(xs) == 0:  # no operand to take ElemT from
            return self.konst(shape, 0.0)
        d, r = dims_arr(shape)
        h = _out()
        check(lib().to_sum(len(xs), _arr(xs), r, d, C.byref(h)))
        return DT(h)

    def scaleT(self, alpha, x):
        h = _out()
        check(lib().to_scale(float(alpha), x.h, C.byref(h)))
        return DT(h)

    def transp(self, x):
        h = _out()
        check(lib().to_transp(x.h, C.byref(h)))
        return DT(h)

    def sumRows(self, x):
        h = _out()
        check(lib().to_sum_rows(x.h, C.byref(h)))
        return DT(h)

    def mapRows_const(self, len_n, row, like):
        h = _out()
        check(lib().to_map_rows_const(len_n, row.h, like.h, C.byref(h)))
        return DT(h)

    def slice(self, x, index):
        d, r = dims_arr(index)
        h = _out()
        check(lib().to_slice(x.h, r, d, C.byref(h)))
        return DT(h)

    def stack(self, dims_m, rows):
        d, r = dims_arr(dims_m)
        h = _out()
        check(lib().to_stack(r, d, _arr(rows), C.byref(h)))
        return DT(h)

    def mapRows(self, len_n, f, x):
        """General `mapRows` (Types.hs:77-81): host traversal over zero-copy row views."""
        lead = x.shape[:len_n]
        rows = [f(self.slice(x, i)) for i in itertools.product(*[range(d) for d in lead])]
        return self.stack(lead, rows)

    def ixRows(self, len_m, f, x):
        lead = x.shape[:len_m]
        rows = [f(i, self.slice(x, i)) for i in itertools.product(*[range(d) for d in lead])]
        return self.stack(lead, rows)

    def diag(self, rank, x):
        h = _out()
        check(lib().to_diag(rank, x.h, C.byref(h)))
        return DT(h)

    def getDiag(self, x):
        h = _out()
        check(lib().to_get_diag(x.h, C.byref(h)))
        return DT(h)

    def index(self, x, i, sample=0):
        d, _ = dims_arr(i)
        v = C.c_double()
        check(lib().to_index(x.h, d, sample, C.byref(v)))
        return v.value

    def arg_max(self, x):
        """`TT.argMax` (Tensor.hs:291-305): int for an unbatched vector, array of B ints when batched."""
        shape, batch = x._shape()
        out = np.empty(max(batch, 1), dtype=np.int64)   # (filled in place: no per-element conversion for a batch of 10^5 rows)
        check(lib().to_arg_max(x.h, out.ctypes.data_as(C.POINTER(C.c_int64))))
        return out if batch > 0 else int(out[0])

    def arg_min(self, x):
        """`TT.argMin` (Tensor.hs:307-321): int for an unbatched vector, array of B ints when batched."""
        shape, batch = x._shape()
        out = np.empty(max(batch, 1), dtype=np.int64)
        check(lib().to_arg_min(x.h, out.ctypes.data_as(C.POINTER(C.c_int64))))
        return out if batch > 0 else int(out[0])

    def one_hot(self, n, hot, cold, i):
        """`TT.oneHot` (Tensor.hs:275-289); `i` an int (unbatched) or a sequence of B ints."""
        batched = not np.isscalar(i)
        idx = np.ascontiguousarray(i if batched else [i], dtype=np.int64)
        h = _out()
        check(lib().to_one_hot(self.to_dtype, n, float(hot), float(cold), len(idx) if batched else 0,
                               idx.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(h)))
        return DT(h)

    # hidden_act / a stateful layer's state activation: TO_ACT_LOGISTIC, TO_ACT_TANH
    _HIDDEN = {"logistic": 0, "tanh": 3}

    def stack_grad(self, ws, bs, x, y, out_act="softmax", loss="crossEntropy", hidden_act="logistic", want_losses=False):
        """batched parameter gradients of a genNet stack (to_fflayer_stack_grad): (gW list, gb list, losses [B] or None)"""
        gW = [self._alloc(w.shape, 0) for w in ws]
        gB = [self._alloc(b.shape, 0) for b in bs]
        losses = self._alloc((), x.batch) if want_losses else None
        check(lib().to_fflayer_stack_grad(len(ws), _arr(ws), _arr(bs), self._HIDDEN[hidden_act], self._RNN_OUT[out_act],
                                          self._RNN_LOSS[loss], x.h, y.h, _arr(gW), _arr(gB),
                                          losses.h if losses is not None else None))
        return gW, gB, losses

    def stack_sgd(self, ws, bs, x, y, rate, out_act="softmax", loss="crossEntropy", hidden_act="logistic",
                  want_losses=False):
        """the `trainNetwork` step on one batch, parameters updated in place (to_fflayer_stack_sgd)"""
        losses = self._alloc((), x.batch) if want_losses else None
        check(lib().to_fflayer_stack_sgd(len(ws), _arr(ws), _arr(bs), self._HIDDEN[hidden_act], self._RNN_OUT[out_act],
                                         self._RNN_LOSS[loss], x.h, y.h, float(rate),
                                         losses.h if losses is not None else None))
        return losses

    def stack_minibatch_sgd(self, ws, bs, X, Y, rate, minibatch, idx=None, n=None, out_act="softmax", loss="crossEntropy",
                            hidden_act="logistic", want_losses=False):
        """minibatch SGD over rows idx (None: rows 0..n-1, n None: every row) of the resident X / Y, one `trainNetwork` step a
        minibatch, parameters updated in place, in one call (to_fflayer_stack_minibatch_sgd).  Y None: the target of a row
        is the row itself (`trainEncoder`).  The losses [n_idx] of the rows in idx's order if asked for."""
        arr = None
        if idx is not None:
            arr = np.ascontiguousarray(idx, dtype=np.int64)
            n = len(arr) if n is None else n
        elif n is None:
            n = X.batch
        losses = self._alloc((), int(n)) if want_losses and n >= 1 else None
        check(lib().to_fflayer_stack_minibatch_sgd(len(ws), _arr(ws), _arr(bs), self._HIDDEN[hidden_act],
                                                   self._RNN_OUT[out_act], self._RNN_LOSS[loss], X.h,
                                                   Y.h if Y is not None else None, int(n),
                                                   arr.ctypes.data_as(C.POINTER(C.c_int64)) if arr is not None else None,
                                                   int(minibatch), float(rate), losses.h if losses is not None else None))
        return losses

    @staticmethod
    def minibatch_stage_bytes(nbytes):
        """to_set_minibatch_stage_bytes: the bound on the staging buffer of stack_minibatch_sgd (0: the default); returns the
        previous bound"""
        prev = C.c_int64()
        check(lib().to_set_minibatch_stage_bytes(int(nbytes), C.byref(prev)))
        return prev.value

    # -- encoder / decoder pairs (to_autoencoder_stack_*) -----------------------------------------------------------------
    # ws / bs: every layer's parameters in input-to-output order, the first n_enc of them the encoder; code_act the encoder's
    # output activation, (out_act, loss) the reconstruction head; the target of a row is the row itself
    _AE_ACT = {"logistic": 0, "softmax": 2, "tanh": 3, "identity": 4}

    def _ae_args(self, ws, bs, n_enc, hidden_act, code_act, out_act=None, loss=None):
        a = [int(n_enc), len(ws) - int(n_enc), _arr(ws), _arr(bs), self._AE_ACT[hidden_act]]
        if code_act is not None:
            a.append(self._AE_ACT[code_act])
        a.append(self._AE_ACT[out_act])
        if loss is not None:
            a.append(self._RNN_LOSS[loss])
        return a

    def autoencoder_run(self, ws, bs, n_enc, x, out_act="logistic", loss="squaredError", hidden_act="logistic",
                        code_act="logistic", want_code=True, want_recon=True, want_losses=True):
        """`encode`, `encodeDecode` and `testEncoder` over the batch of x (to_autoencoder_stack_run): (code, recon, losses),
        None where not asked for"""
        _, batch = x._shape()
        code = self._alloc((ws[n_enc - 1].shape[0],), batch) if want_code else None
        recon = self._alloc((ws[-1].shape[0],), batch) if want_recon else None
        losses = self._alloc((), batch) if want_losses else None
        check(lib().to_autoencoder_stack_run(*self._ae_args(ws, bs, n_enc, hidden_act, code_act, out_act, loss), x.h,
                                             *[t.h if t is not None else None for t in (code, recon, losses)]))
        return code, recon, losses

    def autoencoder_decode(self, ws, bs, n_enc, code, out_act="logistic", hidden_act="logistic"):
        """`decode` over the batch of code (to_autoencoder_stack_decode)"""
        _, batch = code._shape()
        out = self._alloc((ws[-1].shape[0],), batch)
        check(lib().to_autoencoder_stack_decode(*self._ae_args(ws, bs, n_enc, hidden_act, None, out_act), code.h, out.h))
        return out

    def autoencoder_grad(self, ws, bs, n_enc, x, out_act="logistic", loss="squaredError", hidden_act="logistic",
                         code_act="logistic", want_losses=False):
        """`encGrad` summed over the batch of x (to_autoencoder_stack_grad): (gW list, gb list, losses [B] or None)"""
        gW = [self._alloc(w.shape, 0) for w in ws]
        gB = [self._alloc(b.shape, 0) for b in bs]
        losses = self._alloc((), x.batch) if want_losses else None
        check(lib().to_autoencoder_stack_grad(*self._ae_args(ws, bs, n_enc, hidden_act, code_act, out_act, loss), x.h,
                                              _arr(gW), _arr(gB), losses.h if losses is not None else None))
        return gW, gB, losses

    def autoencoder_sgd(self, ws, bs, n_enc, x, rate, out_act="logistic", loss="squaredError", hidden_act="logistic",
                        code_act="logistic", want_losses=False):
        """`trainEncoder` on one batch, parameters updated in place (to_autoencoder_stack_sgd)"""
        losses = self._alloc((), x.batch) if want_losses else None
        check(lib().to_autoencoder_stack_sgd(*self._ae_args(ws, bs, n_enc, hidden_act, code_act, out_act, loss), x.h,
                                             float(rate), losses.h if losses is not None else None))
        return losses

    def autoencoder_minibatch_sgd(self, ws, bs, n_enc, X, rate, minibatch, idx=None, n=None, out_act="logistic",
                                  loss="squaredError", hidden_act="logistic", code_act="logistic", want_losses=False):
        """stack_minibatch_sgd with Y None for an encoder / decoder pair (to_autoencoder_stack_minibatch_sgd)"""
        arr = None
        if idx is not None:
            arr = np.ascontiguousarray(idx, dtype=np.int64)
            n = len(arr) if n is None else n
        elif n is None:
            n = X.batch
        losses = self._alloc((), int(n)) if want_losses and n >= 1 else None
        check(lib().to_autoencoder_stack_minibatch_sgd(
            *self._ae_args(ws, bs, n_enc, hidden_act, code_act, out_act, loss), X.h, int(n),
            arr.ctypes.data_as(C.POINTER(C.c_int64)) if arr is not None else None, int(minibatch), float(rate),
            losses.h if losses is not None else None))
        return losses

    def stack_online_sgd(self, ws, bs, X, Y, n, rate, idx=None, out_act="softmax", loss="crossEntropy",
                         hidden_act="logistic"):
        """per-sample SGD over rows idx[0..n) (None: rows 0..n-1) of X / Y in one launch, parameters updated in place
        (to_fflayer_stack_online_sgd)"""
        arr = None
        if idx is not None:
            arr = np.ascontiguousarray(idx, dtype=np.int64)
        check(lib().to_fflayer_stack_online_sgd(len(ws), _arr(ws), _arr(bs), self._HIDDEN[hidden_act],
                                                self._RNN_OUT[out_act], self._RNN_LOSS[loss], X.h, Y.h, int(n),
                                                arr.ctypes.data_as(C.POINTER(C.c_int64)) if arr is not None else None,
                                                float(rate)))

    def infer_stack(self, ws, bs, x, out_act="softmax", y=None, want_out=False, want_classes=True, hidden_act="logistic"):
        """`runNetwork` of a genNet stack (logistic or tanh hidden layers) over the batch of x, with `validate` /
        `confusion`'s folds (to_fflayer_stack_infer): (out DT or None, classes int64[B] or None, confusion [n_L, n_L]
        indexed [predicted, actual] or None -- given y only)."""
        act = {"softmax": 2, "logistic": 0}[out_act]
        shape, batch = x._shape()
        rows = max(batch, 1)
        nL = ws[-1].shape[0]
        out = None
        if want_out:
            d, r = dims_arr((nL,))
            h = _out()
            check(lib().to_alloc(self.to_dtype, r, d, batch, C.byref(h)))
            out = DT(h)
        classes = np.empty(rows, dtype=np.int64) if want_classes else None
        conf = np.zeros((nL, nL), dtype=np.int64) if y is not None else None
        i64 = C.POINTER(C.c_int64)
        check(lib().to_fflayer_stack_infer(len(ws), _arr(ws), _arr(bs), self._HIDDEN[hidden_act], act, x.h, y.h if y is not None else None,
                                           out.h if out is not None else None,
                                           classes.ctypes.data_as(i64) if classes is not None else None,
                                           conf.ctypes.data_as(i64) if conf is not None else None))
        return out, classes, conf

    # -- recurrent stacks (to_rnn_stack_*) ----------------------------------------------------
    _RNN_OUT = {"softmax": 2, "logistic": 0}
    _RNN_LOSS = {"crossEntropy": 1, "squaredError": 0}

    def _alloc(self, shape, batch):
        d, r = dims_arr(tuple(shape))
        h = _out()
        check(lib().to_alloc(self.to_dtype, r, d, batch, C.byref(h)))
        return DT(h)

    @classmethod
    def _rnn_arrays(cls, layers):
        """layers: [(s, W', W, b)] or [(s, W', W, b, state_act)] in input-to-output order; s = W' = None for a stateless
        ffLayer.  state_act of a stateful layer: "logistic" (the default; also True) or "tanh"."""
        n = len(layers)
        kinds = []
        for lay in layers:
            sa = lay[4] if len(lay) > 4 else True
            if lay[0] is None:
                if sa not in (True, False, None):
                    raise ValueError("a stateless layer has no state activation")
                kinds.append(-1)
            else:
                if sa in (False, None):
                    raise ValueError("a layer with a state needs a state activation")
                kinds.append(cls._HIDDEN["logistic" if sa is True else sa])
        sact = (C.c_int * n)(*kinds)
        col = [(capi.c_tensor * n)(*[(t.h if t is not None else None) for t in ts]) for ts in zip(*[lay[:4] for lay in layers])]
        return n, sact, col

    @staticmethod
    def _rnn_lens(lens, X):
        """lens (one length per sequence of X) as the int64 host array the ragged entries read"""
        arr = np.ascontiguousarray(lens, dtype=np.int64).reshape(-1)
        if len(arr) != max(X.batch, 1):
            raise ValueError("lens needs one entry per sequence of X")
        return arr

    def rnn_stack_run(self, layers, X, out_act="softmax", want_states=False, hidden_act="logistic", lens=None):
        """`runNetwork` threaded over the T steps of X [B; T, i] (to_rnn_stack_run): (out [B; T, n_L], final states --
        one per layer, None for a stateless one -- or None).  lens: sequence b is steps 0 .. lens[b]-1 of X[b], the rest
        padding (to_rnn_stack_run_ragged): out is zero there and the final states are those after step lens[b]-1."""
        n, sact, (s, ws, w, b) = self._rnn_arrays(layers)
        T, _ = X.shape
        batch = X.batch
        out = self._alloc((T, layers[-1][2].shape[0]), batch)
        finals = [self._alloc((lay[2].shape[0],), batch) if (want_states and lay[0] is not None) else None for lay in layers]
        s_out = (capi.c_tensor * n)(*[(f.h if f is not None else None) for f in finals]) if want_states else None
        if lens is not None:
            arr = self._rnn_lens(lens, X)
            check(lib().to_rnn_stack_run_ragged(n, sact, s, ws, w, b, self._HIDDEN[hidden_act], self._RNN_OUT[out_act], X.h,
                                                arr.ctypes.data_as(C.POINTER(C.c_int64)), out.h, s_out))
            return out, (finals if want_states else None)
        check(lib().to_rnn_stack_run(n, sact, s, ws, w, b, self._HIDDEN[hidden_act], self._RNN_OUT[out_act], X.h, out.h, s_out))
        return out, (finals if want_states else None)

    def rnn_stack_grad(self, layers, X, Y, out_act="softmax", loss="crossEntropy", want_gx=False, want_losses=False,
                       hidden_act="logistic", lens=None):
        """BPTT of the stack summed over the sequences of X (to_rnn_stack_grad): (gs, gws, gw, gb -- lists per layer, None
        for a stateless layer's state entries --, gx [B; T, i] or None, losses [B; T] or None).  lens: the objective
        covers steps t < lens[b] only (to_rnn_stack_grad_ragged); gx and losses are zero at padding."""
        n, sact, (s, ws, w, b) = self._rnn_arrays(layers)
        gS = [self._alloc(lay[0].shape, 0) if lay[0] is not None else None for lay in layers]
        gWS = [self._alloc(lay[1].shape, 0) if lay[1] is not None else None for lay in layers]
        gW = [self._alloc(lay[2].shape, 0) for lay in layers]
        gB = [self._alloc(lay[3].shape, 0) for lay in layers]
        T, i = X.shape
        gx = self._alloc((T, i), X.batch) if want_gx else None
        losses = self._alloc((T,), X.batch) if want_losses else None
        arr = lambda ts: (capi.c_tensor * n)(*[(t.h if t is not None else None) for t in ts])  # noqa: E731
        if lens is not None:
            la = self._rnn_lens(lens, X)
            check(lib().to_rnn_stack_grad_ragged(n, sact, s, ws, w, b, self._HIDDEN[hidden_act], self._RNN_OUT[out_act],
                                                 self._RNN_LOSS[loss], X.h, Y.h, la.ctypes.data_as(C.POINTER(C.c_int64)),
                                                 arr(gS), arr(gWS), arr(gW), arr(gB), gx.h if gx is not None else None,
                                                 losses.h if losses is not None else None))
            return gS, gWS, gW, gB, gx, losses
        check(lib().to_rnn_stack_grad(n, sact, s, ws, w, b, self._HIDDEN[hidden_act], self._RNN_OUT[out_act],
                                      self._RNN_LOSS[loss], X.h, Y.h,
                                      arr(gS), arr(gWS), arr(gW), arr(gB), gx.h if gx is not None else None,
                                      losses.h if losses is not None else None))
        return gS, gWS, gW, gB, gx, losses

    def rnn_stack_sgd(self, layers, X, Y, rate_state, rate_params, out_act="softmax", loss="crossEntropy",
                      want_losses=False, hidden_act="logistic", lens=None):
        """`trainNetwork'` in place (to_rnn_stack_sgd); the per-(sequence, step) losses if asked for.  lens: on the steps
        t < lens[b] only (to_rnn_stack_sgd_ragged)."""
        n, sact, (s, ws, w, b) = self._rnn_arrays(layers)
        losses = self._alloc((X.shape[0],), X.batch) if want_losses else None
        if lens is not None:
            la = self._rnn_lens(lens, X)
            check(lib().to_rnn_stack_sgd_ragged(n, sact, s, ws, w, b, self._HIDDEN[hidden_act], self._RNN_OUT[out_act],
                                                self._RNN_LOSS[loss], X.h, Y.h, la.ctypes.data_as(C.POINTER(C.c_int64)),
                                                float(rate_state), float(rate_params),
                                                losses.h if losses is not None else None))
            return losses
        check(lib().to_rnn_stack_sgd(n, sact, s, ws, w, b, self._HIDDEN[hidden_act], self._RNN_OUT[out_act],
                                     self._RNN_LOSS[loss], X.h, Y.h,
                                     float(rate_state), float(rate_params), losses.h if losses is not None else None))
        return losses

    @staticmethod
    def rnn_persistent(on):
        """to_set_rnn_persistent: 0 per step, 1 automatic, 2 wherever in range; returns the previous setting"""
        prev = C.c_int()
        check(lib().to_set_rnn_persistent(int(on), C.byref(prev)))
        return prev.value

    @staticmethod
    def rnn_stats():
        p, q = C.c_int64(), C.c_int64()
        check(lib().to_rnn_stats(C.byref(p), C.byref(q)))
        return p.value, q.value

    @staticmethod
    def rnn_ragged_stats():
        """(persistent runs, per-step runs) of the ragged entries (to_rnn_ragged_stats)"""
        p, q = C.c_int64(), C.c_int64()
        check(lib().to_rnn_ragged_stats(C.byref(p), C.byref(q)))
        return p.value, q.value

    _RNN_FEED = {"output": 0, "argmax": 1, "sample": 2}

    def rnn_stack_generate(self, layers, X, G, feed="output", U=None, out_act="softmax", hidden_act="logistic",
                           want_prime_out=False, want_states=False):
        """Closed-loop generation (to_rnn_stack_generate): prime the stack with X [B; Tp, i], then G steps each fed from
        the step before's output -- as stored ("output"), its argMax one-hot ("argmax") or a symbol drawn by inverse CDF
        with the uniforms U [B; G] ("sample").  Returns (out [B; G, n_L], symbols int64 [B, G] or None, prime_out
        [B; Tp, n_L] or None, final states -- one per layer, None for a stateless one -- or None)"""
        n, sact, (s, ws, w, b) = self._rnn_arrays(layers)
        Tp, _ = X.shape
        batch = X.batch
        nL = layers[-1][2].shape[0]
        G = int(G)
        out = self._alloc((max(G, 1), nL), batch)
        prime = self._alloc((Tp, nL), batch) if want_prime_out else None
        finals = [self._alloc((lay[2].shape[0],), batch) if (want_states and lay[0] is not None) else None for lay in layers]
        s_out = (capi.c_tensor * n)(*[(f.h if f is not None else None) for f in finals]) if want_states else None
        symbols = np.empty((max(batch, 1), max(G, 0)), dtype=np.int64) if feed != "output" else None
        check(lib().to_rnn_stack_generate(n, sact, s, ws, w, b, self._HIDDEN[hidden_act], self._RNN_OUT[out_act],
                                          self._RNN_FEED[feed], X.h, U.h if U is not None else None, G,
                                          prime.h if prime is not None else None, out.h,
                                          symbols.ctypes.data_as(C.POINTER(C.c_int64)) if symbols is not None else None,
                                          s_out))
        return out, symbols, prime, (finals if want_states else None)

    @staticmethod
    def rnn_generate_persistent(on):
        """to_set_rnn_generate_persistent: 0 per step, 1 automatic, 2 wherever in range; returns the previous setting"""
        prev = C.c_int()
        check(lib().to_set_rnn_generate_persistent(int(on), C.byref(prev)))
        return prev.value

    @staticmethod
    def rnn_generate_stats():
        """(persistent runs, per-step runs)"""
        p, q = C.c_int64(), C.c_int64()
        check(lib().to_rnn_generate_stats(C.byref(p), C.byref(q)))
        return p.value, q.value

    def rnn_stack_online_sgd(self, layers, X, Y, rate_state, rate_params, idx=None, n_idx=None, out_act="softmax",
                             loss="crossEntropy", hidden_act="logistic", want_losses=False):
        """`trainNetwork'` folded over the sequences idx[0 .. n_idx) (None: sequences 0 .. n_idx-1, all of them when n_idx is
        None too) of X [N; T, i] / Y [N; T, n_L], one sequence an update, parameters and initial states updated in place
        (to_rnn_stack_online_sgd); the losses [n_idx; T] if asked for"""
        n, sact, (s, ws, w, b) = self._rnn_arrays(layers)
        arr = None
        if idx is not None:
            arr = np.ascontiguousarray(idx, dtype=np.int64)
            n_idx = len(arr) if n_idx is None else n_idx
        elif n_idx is None:
            n_idx = X.batch
        n_idx = int(n_idx)
        losses = self._alloc((X.shape[0],), n_idx) if want_losses and n_idx >= 1 else None
        check(lib().to_rnn_stack_online_sgd(n, sact, s, ws, w, b, self._HIDDEN[hidden_act], self._RNN_OUT[out_act],
                                            self._RNN_LOSS[loss], X.h, Y.h, n_idx,
                                            arr.ctypes.data_as(C.POINTER(C.c_int64)) if arr is not None else None,
                                            float(rate_state), float(rate_params), losses.h if losses is not None else None))
        return losses

    @staticmethod
    def rnn_online_persistent(on):
        """to_set_rnn_online_persistent: 0 per sequence, 1 automatic, 2 wherever in range; returns the previous setting"""
        prev = C.c_int()
        check(lib().to_set_rnn_online_persistent(int(on), C.byref(prev)))
        return prev.value

    @staticmethod
    def rnn_online_stats():
        """(persistent runs, per-sequence runs)"""
        p, q = C.c_int64(), C.c_int64()
        check(lib().to_rnn_online_stats(C.byref(p), C.byref(q)))
        return p.value, q.value

    def rnn_stack_online_sgd_ragged(self, layers, X, Y, lens, rate_state, rate_params, idx=None, n_idx=None,
                                    out_act="softmax", loss="crossEntropy", hidden_act="logistic", want_losses=False):
        """rnn_stack_online_sgd for sequences of their own lengths (to_rnn_stack_online_sgd_ragged): step j trains on steps
        0 .. lens[idx[j]]-1 of its sequence, the rest of its rows is padding and never read.  lens has one entry per
        sequence of X, whatever idx names.  The losses [n_idx; T], zero at padding, if asked for"""
        n, sact, (s, ws, w, b) = self._rnn_arrays(layers)
        la = self._rnn_lens(lens, X)
        arr = None
        if idx is not None:
            arr = np.ascontiguousarray(idx, dtype=np.int64)
            n_idx = len(arr) if n_idx is None else n_idx
        elif n_idx is None:
            n_idx = X.batch
        n_idx = int(n_idx)
        losses = self._alloc((X.shape[0],), n_idx) if want_losses and n_idx >= 1 else None
        check(lib().to_rnn_stack_online_sgd_ragged(n, sact, s, ws, w, b, self._HIDDEN[hidden_act], self._RNN_OUT[out_act],
                                                   self._RNN_LOSS[loss], X.h, Y.h, la.ctypes.data_as(C.POINTER(C.c_int64)),
                                                   n_idx,
                                                   arr.ctypes.data_as(C.POINTER(C.c_int64)) if arr is not None else None,
                                                   float(rate_state), float(rate_params),
                                                   losses.h if losses is not None else None))
        return losses

    @staticmethod
    def rnn_online_ragged_stats():
        """(persistent runs, per-sequence runs) of the ragged entry (to_rnn_online_ragged_stats)"""
        p, q = C.c_int64(), C.c_int64()
        check(lib().to_rnn_online_ragged_stats(C.byref(p), C.byref(q)))
        return p.value, q.value

    # -- induceNetwork iterated (to_fflayer_stack_induce) ----------------------------------------
    def induce_stack(self, ws, bs, x, y, rate, iters, out_act="softmax", loss="crossEntropy", want_gx=False,
                     want_losses=False, in_place=False, hidden_act="logistic"):
        """`induceNetwork` applied `iters` times to every row of x with the parameters fixed (to_fflayer_stack_induce):
        (out -- x itself when in_place --, gx of the last iteration or None, losses [B; iters] or None)"""
        shape, batch = x._shape()
        out = x if in_place else self._alloc(shape, batch)
        gx = self._alloc(shape, batch) if want_gx else None
        losses = self._alloc((iters,), batch) if want_losses else None
        check(lib().to_fflayer_stack_induce(len(ws), _arr(ws), _arr(bs), self._HIDDEN[hidden_act], self._RNN_OUT[out_act],
                                            self._RNN_LOSS[loss],
                                            x.h, y.h, float(rate), int(iters), out.h,
                                            gx.h if gx is not None else None, losses.h if losses is not None else None))
        return out, gx, losses

    @staticmethod
    def induce_persistent(on):
        """to_set_induce_persistent: 0 per iteration, 1 automatic, 2 wherever in range; returns the previous setting"""
        prev = C.c_int()
        check(lib().to_set_induce_persistent(int(on), C.byref(prev)))
        return prev.value

    @staticmethod
    def induce_stats():
        """(persistent runs, per-iteration runs)"""
        p, q = C.c_int64(), C.c_int64()
        check(lib().to_induce_stats(C.byref(p), C.byref(q)))
        return p.value, q.value

    def persist_plan(self, kernel, dims, B=1, iters=1, dtype=None):
        """Debug (to_persist_plan_query): the plan of the online SGD kernel (`kernel` "online") or of the persistent induce
        kernel ("induce") for the stack of widths `dims`, running neither.  "exists" False: the kernel refuses the stack"""
        dt = self.to_dtype if dtype is None else (capi.TO_F64 if dtype in ("f64", capi.TO_F64) else capi.TO_F32)
        d = (C.c_int64 * 8)(*[int(v) for v in dims])
        ex, g, sl, last, ok = C.c_int(), C.c_int(), C.c_int(), C.c_int(), C.c_int()
        lds, grid = C.c_int64(), C.c_int64()
        check(lib().to_persist_plan_query(("online", "induce").index(kernel), dt, len(dims) - 1, d, int(B), int(iters),
                                          C.byref(ex), C.byref(g), C.byref(sl), C.byref(last), C.byref(lds), C.byref(grid),
                                          C.byref(ok)))
        return {"exists": bool(ex.value), "G": g.value, "slice": sl.value, "last_slice": last.value, "lds_bytes": lds.value,
                "grid": grid.value, "placement_ok": bool(ok.value)}

    # -- batching -------------------------------------------------------------------------
    def batch_sum(self, x):
        h = _out()
        check(lib().to_batch_sum(x.h, C.byref(h)))
        return DT(h)

    def batch_bcast(self, x, b):
        h = _out()
        check(lib().to_batch_bcast(x.h, b, C.byref(h)))
        return DT(h)

    def batch_slice(self, x, start, count):
        h = _out()
        check(lib().to_batch_slice(x.h, start, count, C.byref(h)))
        return DT(h)

    def batch_gather(self, x, idx):
        arr = np.ascontiguousarray(idx, dtype=np.int64) if len(idx) else np.zeros(1, dtype=np.int64)
        h = _out()
        check(lib().to_batch_gather(x.h, len(idx), arr.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(h)))
        return DT(h)

    def batch_select(self, x, i):
        h = _out()
        check(lib().to_batch_select(x.h, i, C.byref(h)))
        return DT(h)

    # -- runtime ------------------------------------------------------------------------------
    def force(self, x):
        """`rnf` of one value: its storage exists afterwards (enqueued, not waited for)."""
        check(lib().to_force(x.h))
        return x

    def force_many(self, xs):
        """`rnf` of a product of values, planned together (to_force_many)."""
        xs = list(xs)
        check(lib().to_force_many(len(xs), _arr(xs)))
        return xs

    def sync(self):
        check(lib().to_sync())

    def stats(self):
        a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
        check(lib().to_stats(C.byref(a), C.byref(b), C.byref(c)))
        return {"live_handles": a.value, "pool_bytes": b.value, "launches": c.value}

    def gemm_route(self, m, k, n, dtype="f32", batch=1, reduce_batch=False, a_transposed=False, b_transposed=False,
                   epilogue=()):
        """Debug (to_gemm_route_query): where the contraction [m, k] . [k, n] would go, launching nothing.  `epilogue`: names
        out of bias / act / dact / beta / rowsum.  "families": the kernel family of each launch, in order (None: the library
        would refuse the problem)."""
        cap = 64
        fam = (C.c_int * cap)()
        nl, ok, small, ws = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        bits = sum(capi.GEMM_EPILOGUE_BITS[e] for e in epilogue)
        check(lib().to_gemm_route_query(capi.TO_F64 if dtype in ("f64", capi.TO_F64) else capi.TO_F32, m, n, k,
                                        batch, int(reduce_batch), int(a_transposed), int(b_transposed), bits, cap, fam,
                                        C.byref(nl), C.byref(ok), C.byref(small), C.byref(ws)))
        return {"families": None if nl.value < 0 else [capi.GEMM_FAMILIES[fam[i]] for i in range(nl.value)],
                "epilogue_ok": bool(ok.value), "small_route": bool(small.value), "split_workspace": bool(ws.value)}

    def ewise_route(self, total, n_inputs, family="functor", periods=None, aligned=True, dtype=None):
        """Debug (to_ewise_route_query): (form, blocks, second piece?) of an elementwise launch, launching nothing."""
        dt = self.to_dtype if dtype is None else (capi.TO_F64 if dtype in ("f64", capi.TO_F64) else capi.TO_F32)
        per = None if periods is None else (C.c_int64 * max(len(periods), 1))(*[int(p) for p in periods])
        form, blocks, second = C.c_int(), C.c_int64(), C.c_int()
        check(lib().to_ewise_route_query(dt, n_inputs, int(total), int(bool(aligned)), per, capi.EW_FAMILIES.index(family),
                                         C.byref(form), C.byref(blocks), C.byref(second)))
        return capi.EW_FORMS[form.value], blocks.value, bool(second.value)

    def transfer_stats(self):
        v = [C.c_int64() for _ in range(4)]
        check(lib().to_transfer_stats(*[C.byref(x) for x in v]))
        return dict(zip(("staged_calls", "staged_bytes", "direct_calls", "direct_bytes"), (x.value for x in v)))

    def memo(self):
        return _Memo()

    def timer_start(self):
        check(lib().to_timer_start())

    def timer_stop(self):
        ms = C.c_float()
        check(lib().to_timer_stop(C.byref(ms)))
        return ms.value


class _Memo:
    def __enter__(self):
        check(lib().to_memo_begin())

    def __exit__(self, *a):
        check(lib().to_memo_end())


class Graph:
    """Capture everything enqueued inside the `with` block; `launch()` replays it."""

    def __init__(self):
        self.h = None

    def __enter__(self):
        check(lib().to_graph_begin())
        return self

    def __exit__(self, et, ev, tb):
        g = capi.c_graph()
        st = lib().to_graph_end(C.byref(g))
        if et is None:
            check(st)
        self.h = g

    def launch(self):
        check(lib().to_graph_launch(self.h))

    def __del__(self):
        try:
            if self.h:
                lib().to_graph_release(self.h)
        except Exception:
            pass
