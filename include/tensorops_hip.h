/* tensorops_hip.h -- C ABI of the MI355X (gfx950) backend for mstksg/tensor-ops.
 *
 * This is the drop-in boundary: exactly the entry points a Haskell
 * `instance Tensor HipT` (class at src/TensorOps/Types.hs:52-109) or
 * `instance BLAS HipB` (class at src/TensorOps/BLAS.hs:90-173) would bind with
 * `foreign import ccall` (stubs in INTEGRATION.md).  Plain pointers and sizes
 * only; no C++ or torch types.  All citations are relative to the reference
 * repository root.
 *
 * Conventions
 *  - Every function returns `to_status`: 0 = ok, nonzero = error; the message is
 *    in `to_last_error()` (thread-local).  The reference cannot have shape
 *    errors (dims are type-level); here every dim is re-validated and a
 *    mismatch is TO_ERR_SHAPE.
 *  - Tensors are immutable values behind opaque ref-counted handles, matching
 *    the pure class methods: every op returns a NEW handle in `*out`
 *    (refcount 1); inputs are never written.  A Haskell shim wraps handles in
 *    `ForeignPtr` with `to_release` as finaliser.
 *  - Layout: logical row-major, first dim slowest (`genBTensorA`,
 *    src/TensorOps/Backend/BTensor.hs:503-511).  Handles carry dims+strides so
 *    `transp` is a zero-copy view.
 *  - Hidden batch dimension (new capability): a handle may
 *    carry `batch` = B > 0 independent samples of the same logical shape,
 *    stored sample-major.  `batch` = 0 means "one value shared by all samples"
 *    (parameters).  Ops broadcast unbatched operands over the batch.
 *  - Scalars (`ElemT t` / `ElemB b`) cross as `double` and are rounded to the
 *    tensor dtype inside.
 *  - All work is enqueued on ONE HIP stream (`to_set_stream`); functions that
 *    return host data synchronise that stream.  The library is thread-safe
 *    (one global lock), so it can be called from any Haskell capability.
 */
#ifndef TENSOROPS_HIP_H
#define TENSOROPS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default) /* the library is built with -fvisibility=hidden */

typedef int32_t to_status;
typedef struct to_tensor_s* to_tensor; /* opaque, ref-counted */
typedef struct to_expr_s* to_expr;     /* compiled elementwise expression */
typedef struct to_graph_s* to_graph;   /* captured HIP graph */

enum {
  TO_OK = 0,
  TO_ERR_ARG = 1,    /* null pointer, bad enum, bad rank ...            */
  TO_ERR_SHAPE = 2,  /* dims do not satisfy the op's type-level contract */
  TO_ERR_HIP = 3,    /* a HIP runtime call failed                        */
  TO_ERR_STATE = 4,  /* not initialised, capture misuse ...              */
  TO_ERR_UNSUPPORTED = 5
};

/* dtype = `ElemT t` / `ElemB b`.  TO_F32 is the primary type (north_star parity 1e-5, MFMA and
 * fused paths); TO_F64 is what the reference's apps instantiate (`HMat Double`,
 * src/TensorOps/BLAS/HMat.hs:35): every op, fp64-MFMA GEMM, parity 1e-12.  Operands of one op
 * must share a dtype. */
enum { TO_F32 = 0, TO_F64 = 1 };

#define TO_MAX_RANK 8

/* ---- runtime ------------------------------------------------------------------ */
to_status to_init(int device);        /* idempotent; selects the device          */
to_status to_shutdown(void);          /* frees the pool; handles become invalid  */
const char* to_last_error(void);
to_status to_device_count(int* out);
to_status to_set_stream(void* hip_stream); /* NULL = library-owned stream       */
to_status to_get_stream(void** out);
/* `rnf` of NFData (app/Dots.hs:50-53, app/MNIST.hs:233-235) = wait for the stream */
to_status to_sync(void);
/* live handles / bytes held by the pool (leak checks in tests) */
to_status to_stats(int64_t* live_handles, int64_t* pool_bytes, int64_t* kernel_launches);
/* *ab_knobs = 1 in a development build (the A/B knobs of DESIGN.md are compiled in and read from the environment),
 * 0 in a product build, which reads the documented product switches only */
to_status to_build_info(int* ab_knobs);
/* The element type of the instance (`ElemT t`, src/TensorOps/Types.hs:54): values that
 * have no operand to take a dtype from (`sumT []`) and the host shims' constructors use it.
 * TO_F32 by default; TO_F64 selects the fp64 instance (HMat's element type). */
to_status to_set_default_dtype(int dtype);
to_status to_default_dtype(int* dtype);

/* ---- handles -------------------------------------------------------------------- */
to_status to_alloc(int dtype, int rank, const int64_t* dims, int64_t batch, to_tensor* out);
/* non-owning view of caller-owned device memory (e.g. a torch tensor), contiguous */
to_status to_wrap(void* device_ptr, int dtype, int rank, const int64_t* dims, int64_t batch,
                  to_tensor* out);
to_status to_retain(to_tensor t);
to_status to_release(to_tensor t);
to_status to_shape(to_tensor t, int* rank, int64_t* dims /*[TO_MAX_RANK]*/, int64_t* batch);
to_status to_dtype(to_tensor t, int* dtype);
to_status to_is_contiguous(to_tensor t, int* out);
to_status to_data_ptr(to_tensor t, void** out); /* base pointer of the view */
/* host <-> device, logical row-major order (sample-major when batched).
 * `generateA` / `fromList` (src/TensorOps/Tensor.hs:187-197) build on the host
 * and upload once; `toList`/`ixRows` traversals download once.
 * All three are synchronous (on return the bytes are where they go and `host` may be reused or freed).  `host` may be
 * any memory of the process -- a Haskell `Storable` vector, malloc, the stack: the copy engine never touches it.  The
 * bytes pass through the library's own page-locked staging buffers (two 4 MiB chunks, the next chunk's DMA overlapping
 * the CPU copy); memory the caller has page-locked itself (hipHostMalloc / hipHostRegister, a torch pinned tensor) is
 * transferred in place.  TOPS_PINNED_STAGING=0 hands `host` to the runtime's hipMemcpyAsync as rounds 1-4 did -- under
 * several processes sharing one GPU that path returned downloads with pieces of the destination unwritten (DESIGN_HISTORY.md 11.1). */
to_status to_upload(to_tensor t, const void* host, int64_t nbytes);
to_status to_download(to_tensor t, void* host, int64_t nbytes);
to_status to_from_host(int dtype, int rank, const int64_t* dims, int64_t batch,
                       const void* host, to_tensor* out);
/* transfers of caller memory since start: through the staging buffers / in place (caller-pinned or TOPS_PINNED_STAGING=0) */
to_status to_transfer_stats(int64_t* staged_calls, int64_t* staged_bytes, int64_t* direct_calls, int64_t* direct_bytes);
to_status to_fill(int dtype, int rank, const int64_t* dims, int64_t batch, double value,
                  to_tensor* out); /* `TT.konst`, src/TensorOps/Tensor.hs:49-54 */
/* `genRand` (Types.hs:93-96): counter-based generator, seed+element index -> value.
 * dist 0 = uniform[a,b) (`uniformDistr`), 1 = normal(mean a, std-dev b) (`normalDistr`, FeedForward.hs:206),
 * 2 = exponential(rate a), 3 = cauchy(location a, scale b), 4 = laplace(location a, scale b) -- the `ContGen`
 * instances of `statistics` with a closed-form inverse CDF.  Any other `ContGen d` goes the way the reference's
 * own backends go (BTensor.hs:841: `generateA (\_ -> genContVar d g)`): draw on the host, one to_from_host. */
to_status to_rand(int dtype, int rank, const int64_t* dims, int64_t batch, int dist, double a,
                  double b, uint64_t seed, to_tensor* out);

/* ---- class Tensor (src/TensorOps/Types.hs:52-109) --------------------------------- */
/* gmul (Types.hs:60-66): a : ms++os, b : Reverse os ++ ns -> ms++ns,
 * C[m,n] = sum_o A[m,o1..oq] * B[oq..o1,n] (src/Data/Nested.hs:465-472).
 * The three Length witnesses cross as small ints.
 * One product is DEFERRED in every mode, also outside a scope and with TOPS_LAZY=0: `len_o == 0` on two BATCHED operands
 * -- the per-sample outer products `gradTOp` hands back for a weight matrix (src/TensorOps/TOp.hs:86-88), B*o*i numbers
 * whose only use in a gradient is their sum over the batch.  The returned handle has a shape and no storage; to_sum and
 * to_scale of it record behind it; to_batch_sum of it IS to_gmul_batch_sum (one GEMM with K = B); anything else that
 * asks for its elements produces it then (TO_ERR_UNSUPPORTED above TOPS_OUTER_MAX_BYTES).  The operands are read when
 * that happens: the library's own in-place entry points order themselves after such readers, and when either operand
 * is caller-owned memory (to_wrap) outside a scope the product is computed at once instead, so memory the library
 * cannot watch is never read late.  (to_batch_sum, to_gmul, to_sum, to_scale may therefore plan and launch: `safe` imports.) */
to_status to_gmul(int len_m, int len_o, int len_n, to_tensor a, to_tensor b, to_tensor* out);
/* liftT (Types.hs:56-59): n-ary elementwise map of a compiled expression */
to_status to_lift(to_expr f, int n, const to_tensor* xs, to_tensor* out);
/* sumT (Types.hs:69): left fold of n same-shaped tensors; n == 0 -> zeros of
 * (rank, dims), the `SingI o` evidence (src/Data/List/Util.hs:7-10) */
to_status to_sum(int n, const to_tensor* xs, int rank, const int64_t* dims, to_tensor* out);
to_status to_scale(double alpha, to_tensor x, to_tensor* out); /* scaleT (Types.hs:70) */
to_status to_transp(to_tensor x, to_tensor* out);               /* transp (Types.hs:71-73), zero-copy */
to_status to_sum_rows(to_tensor x, to_tensor* out);             /* sumRows (Types.hs:82-84) */
/* mapRows (Types.hs:77-81) with a constant function -- the only use on the hot
 * path (`TO.sumRows` gradient, src/TensorOps/TOp.hs:155-158): every ms-slice
 * under `like`'s leading `len_n` dims := row */
to_status to_map_rows_const(int len_n, to_tensor row, to_tensor like, to_tensor* out);
/* general mapRows / ixRows (Types.hs:77-81,100-106) are host traversals over
 * zero-copy row views: slice -> user function (device ops) -> stack */
to_status to_slice(to_tensor x, int len_m, const int64_t* index, to_tensor* out);
to_status to_stack(int rank_m, const int64_t* dims_m, const to_tensor* rows, to_tensor* out);
to_status to_diag(int rank, to_tensor x, to_tensor* out);     /* diag (Types.hs:85-88) */
to_status to_get_diag(to_tensor x, to_tensor* out);           /* getDiag (Types.hs:89-92) */
to_status to_index(to_tensor x, const int64_t* index, int64_t sample, double* out); /* (!) (Types.hs:107-109) */
/* `TT.argMax` (src/TensorOps/Tensor.hs:291-305) of a vector, per sample when batched: the
 * index of the maximum, EARLIEST index on ties (`Max (Arg x j)` keeps its left argument).
 * NaN: the result is that left fold's (`a >= b` is false for either NaN, so a NaN is taken and its successor replaces
 * it): n - 1 if the last element is NaN, else the earliest maximum of the elements behind the last NaN -- a function of
 * the row alone, whatever its length or layout.  to_arg_min likewise.
 * Writes max(batch,1) indices to host memory (one download instead of the reference's
 * per-element `ixRows` traversal, Tensor.hs:220-230). */
to_status to_arg_max(to_tensor x, int64_t* host_out);
/* `TT.argMin` (Tensor.hs:307-321): same, minimum; ties -> the earliest index (Min over Arg keeps the left) */
to_status to_arg_min(to_tensor x, int64_t* host_out);
/* `TT.oneHot` (Tensor.hs:275-289) for a batch of indices: out[b][j] = (j == idx[b]) ? hot : cold */
to_status to_one_hot(int dtype, int64_t n, double hot, double cold, int64_t batch,
                     const int64_t* host_idx, to_tensor* out);

/* ---- class BLAS (src/TensorOps/BLAS.hs:90-173); rank-1/2 handles only ------------- */
to_status to_blas_axpy(double alpha, to_tensor x, to_tensor y_or_null, to_tensor* out); /* :97-101 */
to_status to_blas_dot(to_tensor x, to_tensor y, double* out);                           /* :102-104 */
to_status to_blas_ger(to_tensor x, to_tensor y, to_tensor* out);                        /* :108-110 */
to_status to_blas_gemv(double alpha, to_tensor a, to_tensor x, double beta,
                       to_tensor y_or_null, to_tensor* out);                           /* :111-116 */
to_status to_blas_gemm(double alpha, to_tensor a, to_tensor b, double beta,
                       to_tensor c_or_null, to_tensor* out);                           /* :118-123 */
to_status to_blas_scale(double alpha, to_tensor x, to_tensor* out);                     /* scaleB :124-127 */
to_status to_blas_add(to_tensor x, to_tensor y, to_tensor* out);                        /* addB :128 */
to_status to_blas_index_row(int64_t i, to_tensor a, to_tensor* out);                    /* indexRowB :133-136 */
to_status to_blas_transp(to_tensor a, to_tensor* out);                                  /* transpB :137-139 */
to_status to_blas_eye(int dtype, int64_t n, to_tensor* out);                            /* eye :160-161 */
to_status to_blas_trace(to_tensor a, double* out);                                      /* traceB :162-164 */
to_status to_blas_diag(to_tensor x, to_tensor* out);                                    /* diagB :165-167 */
to_status to_blas_get_diag(to_tensor a, to_tensor* out);                                /* getDiagB :168-170 */
to_status to_blas_sum(to_tensor x, double* out);                                        /* sumB :171-173 */
/* liftB (:92-96) = to_lift; indexB (:129-132) = to_index; iRowsB/iElemsB/bgenA/
 * bgenRowsA (:140-159) are host traversals built from to_download/to_from_host. */

/* ---- elementwise expressions ("reified closures") ---------------- */
/* SSA program: value v < arity is input v; value arity+i is the result of
 * instruction i = {op, a, b}; TO_X_CONST takes consts[a].  The last value is
 * the result.  `RealFloat`-polymorphic closures (Types.hs:114-117) are reified
 * by instantiating them at a symbolic element type that emits this code. */
enum {
  TO_X_CONST = 0, TO_X_ADD, TO_X_SUB, TO_X_MUL, TO_X_DIV, TO_X_NEG, TO_X_RECIP, TO_X_EXP,
  TO_X_LOG, TO_X_SQRT, TO_X_ABS, TO_X_SIGNUM, TO_X_SIN, TO_X_COS, TO_X_TANH, TO_X_POW,
  TO_X_MAX, TO_X_MIN, TO_X_NOPS
};
to_status to_expr_compile(int arity, int n_instr, const int32_t* code /*[3*n_instr]*/,
                          int n_consts, const double* consts, to_expr* out);
to_status to_expr_release(to_expr e);
/* which kernel runs it: 0 = bytecode VM, 1..99 = a pre-fused functor, 100 = a kernel specialised
 * for this program at run time (hiprtc; TOPS_EXPR_JIT=0 disables) */
to_status to_expr_kind(to_expr e, int* kind);
/* Semantics of the piecewise opcodes, the same in every evaluator ("Elementwise semantics"): TO_X_ABS clears the
 * sign bit (abs(-0.0) = +0.0); TO_X_SIGNUM returns a zero or a NaN operand as it is; TO_X_MAX is `a <= b ? b : a` and
 * TO_X_MIN is `a <= b ? a : b`, the defaults of the reference's `Ord` -- with a NaN operand max gives the first operand
 * and min the second. */
/* Debug: which kernel form an elementwise launch of `total` output elements over `n_inputs` operands takes, and on how
 * many workgroups of 256 threads, without launching anything.  `periods[i]` is operand i's element count (`total` when it
 * is full-size, less for an unbatched operand broadcast under batched ones; NULL: all full-size); `all_16b_aligned`: the
 * result and every operand start on a 16-byte boundary.  `family` is who evaluates the program: a pre-fused functor, a
 * run-time specialised kernel, or the bytecode VM.  *second_piece: in the stream form, whether any thread handles a second
 * 16-byte piece in its trip.  total == 0 gives *blocks = 0 (no launch).  TO_ERR_STATE before to_init. */
enum { TO_EW_FAMILY_FUNCTOR = 0, TO_EW_FAMILY_JIT = 1, TO_EW_FAMILY_VM = 2 };
enum { TO_EW_FORM_SCALAR = 0, TO_EW_FORM_VEC = 1, TO_EW_FORM_STREAM = 2 };
to_status to_ewise_route_query(int dtype, int n_inputs, int64_t total, int all_16b_aligned, const int64_t* periods,
                               int family, int* form, int64_t* blocks, int* second_piece);

/* ---- batching extension (G = sum_b gradTOp(x_b, p, y_b)) ---------- */
to_status to_batch_sum(to_tensor x, to_tensor* out);     /* [B; ns] -> ns, sum over samples */
to_status to_batch_bcast(to_tensor x, int64_t batch, to_tensor* out); /* ns -> [B; ns] */
to_status to_batch_select(to_tensor x, int64_t sample, to_tensor* out); /* view of one sample */
/* zero-copy view of samples [start, start+count) (a `V.splitAt` chunk, app/MNIST.hs:319) */
to_status to_batch_slice(to_tensor x, int64_t start, int64_t count, to_tensor* out);
/* out[k] = x[idx[k]]: a re-ordered / sub-sampled data set in one pass (the `uniformShuffle`d
 * queue, app/MNIST.hs:308); idx is host memory */
to_status to_batch_gather(to_tensor x, int64_t n_idx, const int64_t* host_idx, to_tensor* out);
/* gmul followed by the sum over samples, fused (the cotangent of an unbatched
 * operand): out = sum_b gmul(a_b, b_b); e.g. dW = sum_b dz_b (x) x_b = dZ^T X */
to_status to_gmul_batch_sum(int len_m, int len_o, int len_n, to_tensor a, to_tensor b,
                            to_tensor* out);

/* ---- purity-based CSE and graph replay ---------------------------------------------- */
/* Inside a memo scope a pure op called again with the same input handles
 * returns the same result handle (values are immutable, so this is exact); it
 * removes the reference's forward recomputation (Types.hs:155). */
to_status to_memo_begin(void);
to_status to_memo_end(void);
/* The scope is also a FUSION scope, and it belongs to the calling thread.  Inside it the pure class methods
 * (to_gmul, to_gmul_batch_sum, to_lift, to_sum, to_scale, to_sum_rows, to_map_rows_const, to_batch_sum,
 * to_fill; to_transp and the slicing views of their results) validate their shapes and return at once with a
 * DEFERRED handle: the op is recorded, nothing is launched.  The recorded graph runs -- with bias, activation,
 * loss head, row sums and the `p - r*g` update folded into the GEMM launches where the kernels allow -- when a
 * value is needed: to_download / to_index / to_data_ptr / any eager entry point taking it, to_force,
 * to_force_many, to_copy_into (which lets the source be produced straight into the destination).  Closing a scope,
 * ending a capture and to_sync demand NOTHING: a handle that is still deferred then stays deferred and is produced when it is asked for (under
 * a garbage collector every intermediate of a step is still "held" until its finaliser has run; launching those
 * would re-run the step unfused).  So a host forces what a step produces -- all of it in ONE to_force_many call,
 * which plans the results together -- before it closes the scope.  Results nobody asks for are never computed
 * (call-by-need, like the reference).  What a value IS never changes; only when it is computed does.  Caller-owned memory (to_wrap) read by recorded ops must not be changed behind the
 * library's back while deferred results derived from it are alive; the library's own in-place entry points
 * (to_upload, to_copy_into, to_sgd_step_inplace, to_comm_allreduce_sum ...) order themselves after such
 * readers.  TOPS_LAZY=0 makes every call eager again. */
/* Numerical contract of the fused loss heads.  A recognised head (found by evaluating the recorded row-local subgraph
 * on three random rows against the closed forms the kernel carries, z in [-2, 2], targets in [0.05, 1.05], agreement to
 * 1e-9; only programs without abs/signum/max/min/pow are considered, so agreement on random points means identity) runs
 * as DIFFERENT CODE from the ops it replaces: softmax >>> crossEntropy's backward as softmax(z) * sum(y) - y with the
 * row maximum subtracted before exp and its loss as sum y (lse - (z - max z)), lse = log sum exp(z - max z); logistic >>>
 * squaredError's as -2 (y - s) s (1 - s) and sum (y - s)^2.  Wherever the recorded ops are finite the two agree within
 * rounding, the gradient AND the loss (tests hold the fused step to 1e-5 / 1e-11 of the fp64 oracle); beyond the range of a
 * literal evaluation (a logit above ln(max float): 88.7 in fp32, 709.8 in fp64) the fused head returns the limit value of
 * the same formulas where the recorded ops -- and the reference -- return inf/NaN
 * (tests/test_gpu_lazy.py::test_extreme_logits_state_the_loss_heads_contract).  The loss is written on lse, not on
 * log(p), so that it stays finite where p = exp(z - max z) / sum underflows (logits further apart than about 87 in fp32, where
 * denormal results are flushed, and 745 in fp64): -y log(p) is NaN or inf there.  Every softmax row head of the library
 * -- the fused one, loss_grad_rows, the online recurrent head, the induce head, the reconstruction head -- takes the one
 * term (csrc/devmath.hpp: ce_term) and is held to one fp64 reference, route by route (tests/test_gpu_heads.py).  What stays
 * non-finite is arithmetic, the same in the reference's: a -inf logit under a zero target (0 * inf = NaN; +inf under any
 * other target), and inf - inf -- a +inf logit, a row that is -inf throughout -- which like a NaN logit makes the whole row
 * NaN; a NaN target makes its row's cotangent and loss NaN and no other row's. */
/* switch for the deferral on the CALLING THREAD (default: TOPS_LAZY, on); returns the previous setting */
to_status to_set_lazy(int on, int* previous_or_null);
/* The loss-head recognition above is an identity test, not a proof; a host that prefers the recorded ops as they are (a row
 * program, or one launch per op) turns it off -- for everything planned from now on, process-wide (default: TOPS_LOSS_HEAD_MATCH,
 * on); returns the previous setting.  Plans cached under the other setting are not reused. */
to_status to_set_loss_head_match(int on, int* previous_or_null);
/* `rnf` of ONE value for a lazy host (`instance NFData (HipT ns)`): make t's storage exist (enqueue, not wait) */
to_status to_force(to_tensor t);
/* `rnf` of a product of values (the new parameters of a training step): one plan, so that launches shared between
 * them -- a weight gradient and its bias gradient, the pair of weight-gradient GEMMs -- are shared */
to_status to_force_many(int n, const to_tensor* ts);
/* counters since start: ops recorded, fused GEMM launches, recorded ops that never got storage of their own, plans */
to_status to_lazy_stats(int64_t* recorded, int64_t* fused_launches, int64_t* elided, int64_t* flushes);
/* host time spent planning / in plans + their launches, nanoseconds since start */
to_status to_lazy_time(int64_t* plan_ns, int64_t* flush_ns);
/* The plan cache: a scope that records the same graph as an earlier one (same ops, wiring, operand layouts, aliasing,
 * demands -- a training loop) reuses that plan instead of planning again; nothing the host has to do.  TOPS_PLAN_CACHE=0
 * turns it off.  Counters since start / drop every cached plan. */
to_status to_plan_cache_stats(int64_t* hits, int64_t* misses, int64_t* entries);
to_status to_plan_cache_clear(void);
/* host time spent inside this library's entry points and how many were called, since start (the rest of a step's
 * host time is the caller's own) */
to_status to_api_time(int64_t* ns, int64_t* calls);
/* Debug: which kernel families a contraction would go to, without launching anything (csrc/gemm_route.cpp).
 * The families are numbered in the order the plan asks them. */
enum {
  TO_GEMM_FAMILY_GEMV = 0,
  TO_GEMM_FAMILY_T32 = 1, /* development builds with TOPS_T32_FIRST=1 only */
  TO_GEMM_FAMILY_SKINNYK = 2,
  TO_GEMM_FAMILY_SKINNYK64 = 3,
  TO_GEMM_FAMILY_KW16 = 4,
  TO_GEMM_FAMILY_KW = 5,
  TO_GEMM_FAMILY_KW64 = 6,
  TO_GEMM_FAMILY_SMALL = 7,
  TO_GEMM_FAMILY_MFMA = 8,
  TO_GEMM_FAMILY_F64 = 9,
  TO_GEMM_FAMILY_NAIVE = 10
};
enum { TO_GEMM_EPI_BIAS = 1, TO_GEMM_EPI_ACT = 2, TO_GEMM_EPI_DACT = 4, TO_GEMM_EPI_BETA = 8, TO_GEMM_EPI_ROWSUM = 16 };
/* The problem: C[m, n] = A[m, k] . B[k, n] of `dtype`, `batch` >= 1 of them (reduce_batch: summed into one C), each operand
 * contiguous or (x_transposed) stored transposed, C contiguous, alpha = 1; `epilogue` is a set of TO_GEMM_EPI_* (BETA:
 * beta = 1 with an addend).  The operands are aligned dummies that nothing dereferences.
 * Out: *n_leaves launches, the first `capacity` of their families in launch order (-1: the library would refuse the
 * problem, to_last_error says why); whether the library fuses an epilogue into this product (*epilogue_ok) and whether
 * its callers hand it to the small-GEMM kernel themselves (*small_route); whether the wave-split kernels' workspace for
 * several workgroups per tile exists (*split_workspace: the placement probe of to_init held).  The last three may be NULL.
 * TO_ERR_STATE before to_init. */
to_status to_gemm_route_query(int dtype, int64_t m, int64_t n, int64_t k, int64_t batch, int reduce_batch, int a_transposed,
                              int b_transposed, int epilogue, int capacity, int* families, int* n_leaves, int* epilogue_ok,
                              int* small_route, int* split_workspace);
/* stream capture of everything enqueued between begin/end into a HIP graph */
to_status to_graph_begin(void);
to_status to_graph_end(to_graph* out);
to_status to_graph_launch(to_graph g);
/* nodes of the captured step, and whether a replay issues them as plain kernel launches (a short step of
 * kernels only: cheaper than hipGraphLaunch on this stack; TOPS_REPLAY_LIST_MAX=0 forces the HIP graph) */
to_status to_graph_info(to_graph g, int* n_launches, int* replays_as_launch_list);
to_status to_graph_release(to_graph g);

/* ---- in-place parameter update (program-level, NOT a class method) ------------------ */
/* p <- p - r*g on caller-owned buffers: the only mutation in the library; used
 * by the replayed training step where parameters live at fixed addresses.
 * Same arithmetic as `stepFunc` (FeedForward.hs:145-147). */
to_status to_sgd_step_inplace(to_tensor p, to_tensor g, double rate);
/* dst <- src on caller-owned storage (lands a freshly computed gradient in the
 * flat buffer the data-parallel all-reduce works on) */
to_status to_copy_into(to_tensor dst, to_tensor src);
/* the same for n (dst, src) pairs in ONE launch (landing every parameter gradient of a step) */
to_status to_copy_into_many(int n, const to_tensor* dsts, const to_tensor* srcs);

/* ---- data-parallel exchange ---------------------------------------- */
/* One process per GPU.  Rank 0 calls to_comm_unique_id and hands the 128 bytes to every rank over any
 * transport the host has; every rank then calls to_comm_init(rank, world, id).  to_comm_allreduce_sum
 * sums a contiguous tensor (the flat gradient buffer) over all ranks in place, enqueued on the library
 * stream (RCCL over xGMI; librccl.so is loaded on first use, TOPS_RCCL_LIB overrides the path). */
to_status to_comm_unique_id(void* out_128_bytes);
to_status to_comm_init(int rank, int world, const void* id_128_bytes);
to_status to_comm_allreduce_sum(to_tensor t);
to_status to_comm_world(int* world); /* the ranks RCCL reports for the communicator (ncclCommCount); 0 when none exists */
to_status to_comm_shutdown(void);

/* The same exchange without RCCL: a one-shot two-phase all-reduce over hipIpc-mapped peer buffers (every rank
 * pushes 1/world of its vector to each peer over all xGMI links at once, reduces its own slice in rank order,
 * pushes the sum to everybody).  to_p2p_create allocates this rank's exchange buffer for vectors of up to
 * max_elems elements and returns its 64-byte IPC handle; the ranks all-gather the handles over any transport and
 * call to_p2p_connect(rank, handles[world][64]).  to_p2p_allreduce_sum(g): g <- sum over ranks, in place, one
 * launch on the library stream.  to_p2p_allreduce_sgd: p <- p - rate * sum (the update of FeedForward.hs:141-147
 * in the same launch; g also receives the sum when also_write_g).  Every rank must pass vectors of the same
 * length.  Alignment: a vector whose length is a multiple of 16 bytes is exchanged 16 bytes per lane -- the slice
 * layout of the inbox / outbox has to be the same on every rank, so it is decided by the LENGTH alone -- and its
 * local address (g, and p) must then be 16-byte aligned too: an offset view of a flat buffer that breaks this is
 * TO_ERR_ARG, not a silent slow path (pad the view, or exchange the whole buffer).  A peer that does not show up within TOPS_P2P_TIMEOUT_S (5 s) makes the launch give up:
 * to_p2p_status then reports a nonzero code and further exchanges are refused. */
to_status to_p2p_create(int64_t max_elems, int dtype, int world, void* out_ipc_handle_64_bytes);
to_status to_p2p_connect(int rank, const void* handles_world_x_64_bytes);
to_status to_p2p_allreduce_sum(to_tensor g);
to_status to_p2p_allreduce_sgd(to_tensor p, to_tensor g, double rate, int also_write_g);
to_status to_p2p_status(int* world, int* timed_out_code);
to_status to_p2p_shutdown(void);

/* ---- pre-fused ffLayer stack (program-level, like the two calls above) --------------- */
/* Batched parameter gradients of `genNet` stacks (FeedForward.hs:216-235),
 *   a_l = act_l (W_l a_{l-1} + b_l),  l = 1..n_layers,  loss(a_L, y),
 * summed over the hidden batch of x/y, written into the caller's gW[l] / gb[l]
 * (e.g. views of the flat all-reduce buffer).  Mathematically the same as gradTOp on
 * the generic path; the per-op launches are collapsed into GEMMs with fused epilogues.
 * hidden_act: TO_ACT_LOGISTIC or TO_ACT_TANH (`actMap tanh`: h = tanh(z), backward d * (1 - h^2) on the stored h), one for
 * every non-final layer; (out_act, loss): (TO_ACT_SOFTMAX, TO_LOSS_CROSS_ENTROPY) or (TO_ACT_LOGISTIC,
 * TO_LOSS_SQUARED_ERROR); TO_ACT_TANH is not an output activation (TO_ERR_UNSUPPORTED, nothing written).  A tanh step
 * takes the launches of the logistic step of the same shape.  losses_or_null: per-sample loss [B].
 * This holds for hidden_act of every to_fflayer_stack_* and to_rnn_stack_* entry below. */
enum { TO_ACT_LOGISTIC = 0, TO_ACT_SOFTMAX = 2, TO_ACT_TANH = 3 };
enum { TO_LOSS_SQUARED_ERROR = 0, TO_LOSS_CROSS_ENTROPY = 1 };
to_status to_fflayer_stack_grad(int n_layers, const to_tensor* w, const to_tensor* b, int hidden_act,
                                int out_act, int loss, to_tensor x, to_tensor y, const to_tensor* gw,
                                const to_tensor* gb, to_tensor losses_or_null);
/* The whole `trainNetwork` step (FeedForward.hs:131-148: p <- p - rate * gradTOp ...) of the same stack on
 * one batch, parameters updated in place: the weight-gradient launches subtract rate * gradient in their
 * epilogue, so the step has no separate update launch.  For a single process (data-parallel ranks need the
 * gradient itself for the all-reduce: to_fflayer_stack_grad + to_sgd_step_inplace).  TO_ERR_UNSUPPORTED,
 * with the parameters untouched, when a weight gradient is not in the range of the fused-epilogue kernel. */
to_status to_fflayer_stack_sgd(int n_layers, const to_tensor* w, const to_tensor* b, int hidden_act, int out_act,
                               int loss, to_tensor x, to_tensor y, double rate, to_tensor losses_or_null);

/* Minibatch SGD over a resident data set -- the loop every caller of to_fflayer_stack_sgd writes around it, and `trainEncoder`
 * (AutoEncoder.hs:87-110) over minibatches -- in ONE call.  For k = 0 .. ceil(n_idx / minibatch) - 1, in order: rows
 * idx[k*minibatch .. min((k+1)*minibatch, n_idx)) of X / Y (idx null: rows k*minibatch .. in place) are one batch, and one
 * to_fflayer_stack_sgd step runs on it: p -= rate * (gradient SUMMED over the batch), parameters updated in place.  The last
 * batch may be short.  A step's launches are to_fflayer_stack_sgd's for that batch, bit for bit.
 *   X               [N; i0], contiguous;
 *   Y_or_null       [N; n_L] of X's batch and dtype, contiguous; null: the target of row r is X's row r itself
 *                   (reconstruction; needs n_L == i0, TO_ERR_SHAPE otherwise; nothing is gathered twice for it);
 *   idx_or_null     n_idx entries in [0, N), repeats allowed, also inside one minibatch; the library has its copy when the
 *                   call returns.  Null: n_idx <= N;
 *   losses_or_null  contiguous batched scalar of batch n_idx: losses[j] is the loss of row idx[j] under the parameters its
 *                   step started from, written by the step's loss head itself.
 * hidden_act, (out_act, loss), dtypes and every other rule are to_fflayer_stack_sgd's (an unsupported pair:
 * TO_ERR_UNSUPPORTED).  n_idx < 1 or minibatch < 1: TO_ERR_ARG; an index out of range: TO_ERR_SHAPE.  Every refusal is
 * decided before the first launch -- "a contraction is outside the small-GEMM range" included, for both batch sizes that
 * occur, the full minibatch and the short tail -- so a refused call leaves parameters and losses untouched.  Pending operands
 * are produced first; refused during graph capture (TO_ERR_STATE); keeps no handle; does not block beyond what taking the
 * copy of idx needs (up to 64 KiB of indices ride the pinned ring, stream-ordered; more go through the synchronous staged
 * transfer).
 * Routes.  idx given: the rows of a CHUNK of consecutive steps are gathered into a pool buffer by one launch
 * (csrc/minibatch_stage.hip: X and Y in the same launch, 16-byte pieces per tensor where its rows allow, elements otherwise)
 * and the chunk's steps run on contiguous slabs of it, each starting on a 16-byte boundary; one stream, so the next chunk
 * reuses the buffer without an event.  A chunk is as many steps as fit the stage bound, one at least.  idx null: no staging,
 * the steps run on views of X / Y.
 * to_set_minibatch_stage_bytes: the stage bound, process-wide; 0 restores the default; returns the previous value.  The
 * default, 32 MiB, is a guess that has NOT been measured (tools/minibatch_scan.py reports one-step chunks next to it;
 * DESIGN.md section 3.3). */
to_status to_fflayer_stack_minibatch_sgd(int n_layers, const to_tensor* w, const to_tensor* b, int hidden_act, int out_act,
                                         int loss, to_tensor X, to_tensor Y_or_null, int64_t n_idx,
                                         const int64_t* idx_or_null, int64_t minibatch, double rate,
                                         to_tensor losses_or_null);
to_status to_set_minibatch_stage_bytes(int64_t bytes, int64_t* previous_or_null);

/* ---- encoder / decoder pairs of ffLayer stacks: AutoEncoder.hs in one call ----------------------------------------------- */
/* `Encoder t i o` (AutoEncoder.hs:37-40) as two `genNet` stacks given as ONE per-layer array: w[l] / b[l], l = 0 .. L-1, L =
 * n_enc + n_dec, in input-to-output order as in to_fflayer_stack_*; layers 0 .. n_enc-1 are the encoder ([i0] -> the code
 * [c]), n_enc .. L-1 the decoder ([c] -> [i0]: w[L-1] must have i0 rows, TO_ERR_SHAPE otherwise).  n_enc < 1 or n_dec < 1:
 * TO_ERR_ARG.  Layer l applies
 *   hidden_act   TO_ACT_LOGISTIC or TO_ACT_TANH, every layer but the two below;
 *   code_act     layer n_enc-1, the encoder's output: TO_ACT_LOGISTIC, TO_ACT_TANH or TO_ACT_IDENTITY (a bare `ffLayer`: no
 *                activation in the forward pass, no act' factor in the backward pass);
 *   out_act      layer L-1, with the loss one of (TO_ACT_SOFTMAX, TO_LOSS_CROSS_ENTROPY), (TO_ACT_LOGISTIC,
 *                TO_LOSS_SQUARED_ERROR), (TO_ACT_TANH, TO_LOSS_SQUARED_ERROR), (TO_ACT_IDENTITY, TO_LOSS_SQUARED_ERROR).
 * Anything else: TO_ERR_UNSUPPORTED with nothing written.  The target of a row is the row itself; with a = out_act(z):
 * squaredError = sum (a - x)^2, dz = 2 (a - x) act'(a), act' = a (1 - a) / 1 - a^2 / 1; softmax with crossEntropy as in
 * to_fflayer_stack_grad (dz = p sum(x) - x).  The to_fflayer_stack_* and to_rnn_stack_* entries refuse TO_ACT_IDENTITY and
 * keep refusing TO_ACT_TANH as an output activation.
 *
 * run: `encode` (:42-48), `encodeDecode` (:58-63) and `testEncoder` (:65-81) over the hidden batch of x ([B; i0], or
 * unbatched: one row).  Each output optional, at least one asked for (else TO_ERR_ARG), caller-allocated, contiguous, of x's
 * dtype and batch: code [B; c], recon [B; i0], losses [B].  With only code asked for the decoder is not run; an output's
 * bits do not depend on which others are asked for.  fp32 or fp64, any B, any widths: never TO_ERR_UNSUPPORTED for a valid
 * stack and pair.  Hidden layers go as to_fflayer_stack_infer's; the head -- bias, activation, loss of a row -- is one row
 * launch behind the last GEMM (csrc/recon_head.hip).  Parameters and x are only read: an output that overlaps x, another
 * output or a parameter is TO_ERR_ARG (decode: out against code and the decoder's parameters).  Refused during graph capture
 * (TO_ERR_STATE).
 * decode: `decode` (:50-56): layers n_enc .. L-1 on code [B; c] into out [B; i0]; the encoder's entries of w / b are not
 * looked at.
 * grad: `encGrad` (:112-142) summed over the batch of x ([B; i0], contiguous) into gw[l] / gb[l]; losses[r] = testEncoder of
 * row r.  sgd: `trainEncoder` (:87-110) on one batch, parameters updated in place.  minibatch_sgd:
 * to_fflayer_stack_minibatch_sgd with Y = NULL for these stacks: the same idx, tail-minibatch, losses and staging rules
 * (to_set_minibatch_stage_bytes included).  The three carry exactly the refusals of to_fflayer_stack_grad / _sgd /
 * _minibatch_sgd for the same shapes -- an fp64 contraction outside the small-GEMM range, an sgd weight gradient outside it
 * -- every one decided before the first launch: a refused call leaves parameters, gradients and losses untouched.  When
 * code_act == hidden_act and the pair is one of to_fflayer_stack_grad's two they issue the launches of to_fflayer_stack_grad
 * / _sgd / _minibatch_sgd on (w, b, x, y = x) and produce the same bits; a stack whose code activation is the other of
 * logistic / tanh takes the same number of launches; the pairs with tanh / identity run the row launch of
 * csrc/recon_head.hip behind the last GEMM where the old pairs have their loss head. */
enum { TO_ACT_IDENTITY = 4 };
to_status to_autoencoder_stack_run(int n_enc, int n_dec, const to_tensor* w, const to_tensor* b, int hidden_act, int code_act,
                                   int out_act, int loss, to_tensor x, to_tensor code_or_null, to_tensor recon_or_null,
                                   to_tensor losses_or_null);
to_status to_autoencoder_stack_decode(int n_enc, int n_dec, const to_tensor* w, const to_tensor* b, int hidden_act, int out_act,
                                      to_tensor code, to_tensor out);
to_status to_autoencoder_stack_grad(int n_enc, int n_dec, const to_tensor* w, const to_tensor* b, int hidden_act, int code_act,
                                    int out_act, int loss, to_tensor x, const to_tensor* gw, const to_tensor* gb,
                                    to_tensor losses_or_null);
to_status to_autoencoder_stack_sgd(int n_enc, int n_dec, const to_tensor* w, const to_tensor* b, int hidden_act, int code_act,
                                   int out_act, int loss, to_tensor x, double rate, to_tensor losses_or_null);
to_status to_autoencoder_stack_minibatch_sgd(int n_enc, int n_dec, const to_tensor* w, const to_tensor* b, int hidden_act,
                                             int code_act, int out_act, int loss, to_tensor X, int64_t n_idx,
                                             const int64_t* idx_or_null, int64_t minibatch, double rate,
                                             to_tensor losses_or_null);

/* Per-sample online SGD -- `foldl' (\nt (i,o) -> trainNetwork loss rate i o nt)` (app/MNIST.hs:390-396,
 * app/Dots.hs:74-80) -- of the same stacks over rows idx[0..n_idx) (null: rows 0..n_idx-1) of the resident batched X / Y,
 * parameters updated in place, as ONE persistent launch: the workgroups keep the parameters in LDS between samples,
 * layer 1 split by rows and layer 2 by columns over up to 32 workgroups of one XCD, one exchange per sample
 * (csrc/online_sgd.hip).  hidden_act TO_ACT_LOGISTIC or TO_ACT_TANH; fp32 or fp64, 2..6 layers, input <= 2048, head <= 64 outputs, everything a workgroup holds within
 * 160 KiB of LDS: TO_ERR_UNSUPPORTED otherwise, with the parameters untouched (the generic path -- one recorded and
 * fused step per sample -- always works).  Blocks until the stream of samples is done. */
to_status to_fflayer_stack_online_sgd(int n_layers, const to_tensor* w, const to_tensor* b, int hidden_act, int out_act,
                                      int loss, to_tensor X, to_tensor Y, int64_t n_idx, const int64_t* idx_or_null,
                                      double rate);

/* The same, found by the library itself.  `g` is a captured ONE-SAMPLE training step (whatever the host's DSL recorded
 * in a scope: gradTOp of its network, the update, to_copy_into of the new parameters), x_buf / y_buf the buffers that
 * step reads its sample from.  If the launches the planner made of that step are exactly the trainNetwork step of an
 * ffLayer stack -- GEMVs with bias + logistic (a captured TANH step is not recognised: *handled = 0; call
 * to_fflayer_stack_online_sgd with TO_ACT_TANH instead), a recognised loss head, the cotangents back through the layers, every
 * layer's outer-product update in place -- and the stack fits the persistent kernel, the samples idx[0..n_idx) of X / Y
 * are trained in one launch and *handled = 1; otherwise *handled = 0 and nothing has been done (replay `g` per sample).
 * The host says nothing about what its network is made of.  TOPS_ONLINE_KERNEL=0 disables it. */
to_status to_graph_online_sgd(to_graph g, to_tensor x_buf, to_tensor y_buf, to_tensor X, to_tensor Y, int64_t n_idx,
                              const int64_t* idx_or_null, int* handled);

/* how often to_graph_online_sgd recognised a captured step and ran the persistent kernel, and over how many samples */
to_status to_online_sgd_stats(int64_t* runs, int64_t* samples);

/* `runNetwork` (FeedForward.hs:123-129, 216-235) of the same stacks over the hidden batch of x -- a_l = act_l (W_l a_{l-1}
 * + b_l), hidden_act TO_ACT_LOGISTIC or TO_ACT_TANH, out_act TO_ACT_SOFTMAX or TO_ACT_LOGISTIC -- with the validation folds of
 * app/MNIST.hs:366-389 in the same call.  fp32 or fp64, any batch (an unbatched x is one row), any layer widths: never
 * TO_ERR_UNSUPPORTED for a valid stack.  What it writes, each optional, at least one asked for (else TO_ERR_ARG):
 *   out_or_null        caller-allocated [B; n_L] of x's dtype (contiguous): the network's output rows;
 *   classes_or_null    host int64[B]: `TT.argMax` of every row of out as stored -- bit for bit what to_arg_max returns for
 *                      it, ties (earliest index) and NaN included;
 *   confusion_or_null  host int64[n_L * n_L], [predicted * n_L + actual], actual = argMax of the target row of
 *                      y_or_null ([B; n_L], x's dtype; required for it, TO_ERR_ARG otherwise): `confusion`'s map, its
 *                      trace `validate`'s count of correct rows.
 * Parameters, x and y are only read; pending operands are produced first.  The last layer and everything after it is ONE
 * launch for n_L <= 32 at any fan-in (csrc/infer_head.hip: the activations stream from HBM once, W_L in LDS); wider heads
 * are the last GEMM plus one row launch.  A row's values do not depend on the batch or the row's place in it.  Refused
 * during graph capture (TO_ERR_STATE); blocks when it returns host data; keeps no handle. */
to_status to_fflayer_stack_infer(int n_layers, const to_tensor* w, const to_tensor* b, int hidden_act, int out_act,
                                 to_tensor x, to_tensor y_or_null, to_tensor out_or_null,
                                 int64_t* classes_or_null, int64_t* confusion_or_null);

/* Recurrent stacks (Recurrent.hs): `runNetwork` threaded over T steps, `netGrad` (BPTT, `unroll` >>> `rollup`) summed over
 * the sequences of a hidden batch, and `trainNetwork'`, each ONE call.  Per-layer arrays in input-to-output order, like the
 * ffLayer entries.  Layer l is
 *   state_act[l] == TO_ACT_LOGISTIC   `fullyConnected` (Recurrent.hs:91-119): z = W x + W' s + b, new state logistic(z),
 *                                     output z through the layer's `*~ act`; s[l] [n_l], ws[l] = W' [n_l, n_l];
 *   state_act[l] == TO_ACT_TANH       the same with the new state tanh(z); the layers of one stack mix freely;
 *   state_act[l] == TO_RNN_STATELESS  an ffLayer (Recurrent.hs:126-138); s[l] and ws[l] (and gs[l], gws[l]) null;
 * w[l] = W [n_l, n_{l-1}], b[l] [n_l].  hidden_act (the `*~ act` behind every non-final layer of either kind, whatever its
 * state_act) TO_ACT_LOGISTIC or TO_ACT_TANH; run: out_act TO_ACT_SOFTMAX or TO_ACT_LOGISTIC; grad /
 * sgd: (out_act, loss) (TO_ACT_SOFTMAX, TO_LOSS_CROSS_ENTROPY) or (TO_ACT_LOGISTIC, TO_LOSS_SQUARED_ERROR); anything else
 * is TO_ERR_UNSUPPORTED, nothing written.  The reference's order: `Prod t ss` lists later layers' states first (`~*~`:
 * ss2 ++ ss1) and each fullyConnected carries its parameters as (W', W, b); here layer l's state is s[l] and its parameters
 * ws[l], w[l], b[l] whatever the position.
 * X [B; T, i] (or [T, i]: one sequence): B independent sequences, step 0 consumed first -- plain time order; the
 * reference's reversed order (Recurrent.hs:289-293) is a detail of its netGrad and does not appear here.  Y and out
 * [B; T, n_L] of X's batch.
 *   run   every step's output row into out (contiguous); s_out_or_null[l] (optional per stateful layer, contiguous
 *         [B; n_l] of X's batch) the final state.  s[l] unbatched (every sequence starts from it) or [B; n_l]: the s_out
 *         of one call is the s of the next, a long sequence fed in chunks.
 *   grad  objective sum_b sum_t loss(out_{b,t}, Y_{b,t}); gs / gws / gw / gb get the cotangents of the (unbatched)
 *         initial states and of the parameters; gx_or_null [B; T, i] the per-sequence, per-step input cotangents;
 *         losses_or_null [B; T] the per-(sequence, step) losses.
 *   sgd   `trainNetwork'` in place: s -= rate_state gs, every parameter -= rate_params g.  A refused call updates nothing.
 * Initial states of grad / sgd must be unbatched (TO_ERR_SHAPE).  fp32 or fp64, any B, T >= 1 and widths: never
 * TO_ERR_UNSUPPORTED for a valid stack.  Pending operands are produced first; refused during graph capture (TO_ERR_STATE);
 * blocks before returning; keeps no handle.
 * Routes.  Time-independent work -- input projections, heads, weight gradients, input cotangents -- is one contraction over
 * all B*T rows.  A stateful layer's recurrence is either ONE persistent launch per direction for all T steps
 * (csrc/rnn_seq.hip; its range: n_l <= 1024, fp32 and fp64, any B and T -- the launch count of a call does not depend on T
 * there) or per step (one GEMM with the addend + one elementwise launch per step and direction).  to_set_rnn_persistent:
 * 0 per step; 1 automatic (default): persistent where the kernel holds W' in LDS (fp32 n_l <= 201, fp64 n_l <= 142), the
 * threshold measured in DESIGN.md section 3.3 -- on logistic states; a tanh state takes the same routes by the same
 * threshold, which has NOT been measured for tanh --, per step otherwise; 2 persistent wherever in range.  Process-wide.
 * to_rnn_stats counts the calls with a stateful layer: all of its recurrences persistent, or at least one per step. */
enum { TO_RNN_STATELESS = -1 };
to_status to_rnn_stack_run(int n_layers, const int* state_act, const to_tensor* s, const to_tensor* ws, const to_tensor* w,
                           const to_tensor* b, int hidden_act, int out_act, to_tensor X, to_tensor out,
                           const to_tensor* s_out_or_null);
to_status to_rnn_stack_grad(int n_layers, const int* state_act, const to_tensor* s, const to_tensor* ws, const to_tensor* w,
                            const to_tensor* b, int hidden_act, int out_act, int loss, to_tensor X, to_tensor Y,
                            const to_tensor* gs, const to_tensor* gws, const to_tensor* gw, const to_tensor* gb,
                            to_tensor gx_or_null, to_tensor losses_or_null);
to_status to_rnn_stack_sgd(int n_layers, const int* state_act, const to_tensor* s, const to_tensor* ws, const to_tensor* w,
                           const to_tensor* b, int hidden_act, int out_act, int loss, to_tensor X, to_tensor Y,
                           double rate_state, double rate_params, to_tensor losses_or_null);
to_status to_set_rnn_persistent(int on, int* previous_or_null);
to_status to_rnn_stats(int64_t* persistent_runs, int64_t* stepwise_runs);

/* The same three entries for a batch whose sequences have DIFFERENT lengths (`trainNetwork` of Recurrent.hs takes a list
 * [(x, y)] of any length): the argument list of the dense sibling with `lens` directly after the data tensors.  lens is a
 * host array of B entries (one for X [T, i]) and may be reused on return.  Sequence b is steps 0 .. lens[b]-1 of X[b]; the
 * steps t >= lens[b] are PADDING.  1 <= lens[b] <= T, otherwise TO_ERR_SHAPE; lens null is TO_ERR_ARG.
 *   Padding is never read: padding rows of X and Y may hold anything, NaN and Inf included, and influence no output bit.
 *   run   out[b, t] is the stack's output for t < lens[b] and exactly +0.0 at padding; s_out[l][b] is the state after step
 *         lens[b]-1 -- valid as s of a following dense or ragged call (a ragged batch fed in chunks).
 *   grad  objective sum_b sum_{t < lens[b]} loss(out_{b,t}, Y_{b,t}); gs / gws / gw / gb its cotangents; gx and losses are
 *         exactly +0.0 at padding.
 *   sgd   `trainNetwork'` on that objective, in place.
 * Every other rule is the dense sibling's, with its statuses: the stack, state_act, hidden_act, the (out_act, loss) pairs,
 * the dtypes, the batching of s, the unbatched initial states of grad / sgd, contiguity, refusal during graph capture; every
 * refusal leaves every destination untouched.  fp32 and fp64, any B, T and widths: never TO_ERR_UNSUPPORTED for a valid
 * stack.
 * Routes.  The sequences are sorted by length (descending, stable) and their steps packed time-major: at step t the active
 * sequences own consecutive packed rows, N = sum lens rows in all (csrc/rnn_ragged.hip: one pack launch per data tensor,
 * one unpack launch per [B; T, .] destination, device tables of O(B + T)).  The time-independent work is the dense entries'
 * contractions over exactly N rows, so the work follows sum lens, not B T, and padding enters no contraction.  A stateful
 * layer's recurrence is one persistent launch per direction (rnn_ragged_seq_kernel: a workgroup of short sequences ends
 * early; the launch count depends on neither T nor lens) or per step on the rows still active (launches grow with max lens,
 * not with T).  to_set_rnn_persistent and its threshold (W' in LDS) decide exactly as for the dense entries; that threshold
 * was measured on equal-length batches and HAS NOT BEEN MEASURED for ragged ones.  With every length equal to T the results
 * are the dense entries', bit for bit.  The dense entries, their launches and to_rnn_stats are untouched by these calls;
 * to_rnn_ragged_stats counts the ragged calls with a stateful layer by route.
 * Measured (tools/rnn_ragged_scan.py, profiles/rnn_ragged_scan.txt; fp32, T = 64, lengths uniform in 1..T, grad and sgd
 * alike, persistent route): against the caller's loop of one dense call per distinct length on to_batch_gather'ed groups the
 * ragged call is 2.6x to 21x ahead (5 -> 7 -> 5: 14x at B = 64, 2.7x at B = 1024; 64 -> 128 -> 64: 21x and 13x); against the
 * dense entry on the padded batch (B T rows of work, not the ragged objective) 1.35x / 1.8x ahead on the narrow stack and
 * 0.97x (B = 64: behind) / 1.27x on the wide one -- 2.6x and 1.6x of padded x sum lens / (B T), which it does NOT reach
 * there: the longest sequences' workgroups still walk all their steps.  Where it LOSES: with every length equal to T it is
 * 5 to 12 % behind the dense entry (the table upload, pack and unpack buy nothing then) -- call the dense entry for such a
 * batch.  NOT measured: fp64, tanh states, the per-step route, the persistent / per-step threshold under ragged batches. */
to_status to_rnn_stack_run_ragged(int n_layers, const int* state_act, const to_tensor* s, const to_tensor* ws,
                                  const to_tensor* w, const to_tensor* b, int hidden_act, int out_act, to_tensor X,
                                  const int64_t* lens, to_tensor out, const to_tensor* s_out_or_null);
to_status to_rnn_stack_grad_ragged(int n_layers, const int* state_act, const to_tensor* s, const to_tensor* ws,
                                   const to_tensor* w, const to_tensor* b, int hidden_act, int out_act, int loss, to_tensor X,
                                   to_tensor Y, const int64_t* lens, const to_tensor* gs, const to_tensor* gws,
                                   const to_tensor* gw, const to_tensor* gb, to_tensor gx_or_null, to_tensor losses_or_null);
to_status to_rnn_stack_sgd_ragged(int n_layers, const int* state_act, const to_tensor* s, const to_tensor* ws,
                                  const to_tensor* w, const to_tensor* b, int hidden_act, int out_act, int loss, to_tensor X,
                                  to_tensor Y, const int64_t* lens, double rate_state, double rate_params,
                                  to_tensor losses_or_null);
to_status to_rnn_ragged_stats(int64_t* persistent_runs, int64_t* stepwise_runs);

/* Closed-loop generation of the same stacks in ONE call: `runNetworkSt` under `iterate` -- prime the stack with a few steps,
 * then feed every output back as the next input.  The stack, state_act, hidden_act, out_act (TO_ACT_SOFTMAX or
 * TO_ACT_LOGISTIC; anything else TO_ERR_UNSUPPORTED), the dtypes, the batching of s (unbatched or [B; n_l]) and the s_out
 * rules are to_rnn_stack_run's.  One STEP is what to_rnn_stack_run does for one time step: z = W a + W' s + b, new state
 * state_act(z), layer output hidden_act(z), out_act(z) for the last layer.
 *   prime     X [B; Tp, i] (or [Tp, i]), Tp >= 1: steps 0 .. Tp-1 consume X as to_rnn_stack_run would; their outputs go to
 *             prime_out_or_null, a contiguous [B; Tp, n_L].
 *   generate  for k = 0 .. G-1: x_k = feed(prev_k), prev_0 the last prime output and prev_k = g_{k-1} after that;
 *             g_k = step(x_k) into out, a contiguous [B; G, n_L].  n_L == i is required (TO_ERR_SHAPE), G >= 1 (TO_ERR_ARG).
 *   feed      TO_FEED_OUTPUT  x_k is prev_k as stored;
 *             TO_FEED_ARGMAX  x_k = oneHot(c), c bit for bit what to_arg_max returns for the stored row prev_k (earliest
 *                             index on ties);
 *             TO_FEED_SAMPLE  inverse CDF with the caller's uniforms U, a contiguous [B; G] of X's dtype and batch (to_rand
 *                             makes one).  In the row's dtype and sequentially: c_0 = p_0, c_j = c_{j-1} + p_j,
 *                             thr = U[b, k] * c_{n-1}; the symbol is the number of j with c_j <= thr, at most n - 1.  The
 *                             order and the dtype of these operations are part of the contract: a sequential restatement
 *                             (numpy's cumsum) gives the same symbol from the same stored row.
 *             U is required for TO_FEED_SAMPLE and must be null otherwise (TO_ERR_ARG both ways).
 *   symbols_or_null  host int64[B * G]: symbols[b * G + k] is the index fed at generated step k; the one-hot modes only (with
 *             TO_FEED_OUTPUT it must be null, TO_ERR_ARG).
 *   s_out_or_null[l]  the state after Tp + G steps, a contiguous [B; n_l]: valid as s of a following call.
 * An output that overlaps an input, a parameter or another output is TO_ERR_ARG.  fp32 or fp64, any B, Tp, G and widths:
 * never TO_ERR_UNSUPPORTED for a valid stack.  Pending operands are produced first; refused during graph capture
 * (TO_ERR_STATE); every refusal is decided before the first launch and leaves all outputs untouched; blocks before
 * returning; keeps no handle.
 * Routes.  The generated steps are a dependent chain.  Per step (A): the prime is to_rnn_stack_run's forward on X (its
 * routes, to_set_rnn_persistent), then per generated step one feed launch (csrc/rnn_generate.hip) and that forward with
 * T = 1 on the carried states -- a generated step's values are bit for bit those of to_rnn_stack_run with T = 1 on the fed
 * rows and the carried (batched) states; takes every stack, launches grow with G.  Persistent (B, rnn_gen_kernel): the
 * prime and all G steps of all rows in ONE launch, every layer's W, W' and b in LDS, a workgroup owning whole sequences and
 * the whole stack; the launch count depends neither on Tp nor on G.  The prime runs in the kernel too, so that on either
 * route cutting a generation into two calls (G = a, then one prime row fed from g_{a-1} with the first call's s_out and
 * G = b - 1) gives the bits of the one call with G = a + b.  Its range: 1..8 layers, fp32 and fp64, and the parameters plus
 * one sequence's rows within 160 KiB of LDS -- fp32 64 -> 128 (stateful) -> 64 (129 KiB of parameters) fits, 64 -> 160
 * (stateful) -> 64 (181 KiB) and fp64 64 -> 128 -> 64 (258 KiB) do not and take route A.  Both routes use one definition of
 * the feed rule; on either a row's bits depend neither on B nor on the row's place in the batch; the two routes agree to
 * rounding, not bit for bit.  to_set_rnn_generate_persistent: 0 route A; 1 automatic (default): route B where its plan fits
 * AND the batch fits 256 workgroups with at most four (row, column) items of the widest layer a thread -- B <= 2048 for
 * fp32 64 -> 128 -> 64, every B up to 4096 for 5 -> 7 -> 5 --, route A beyond: measured by tools/rnn_generate_scan.py
 * (profiles/rnn_generate_scan.txt; logistic states and a stateless output layer only); 2 route B
 * wherever its plan fits.  Process-wide.  to_rnn_generate_stats counts calls by the route that ran the generated steps. */
enum { TO_FEED_OUTPUT = 0, TO_FEED_ARGMAX = 1, TO_FEED_SAMPLE = 2 };
to_status to_rnn_stack_generate(int n_layers, const int* state_act, const to_tensor* s, const to_tensor* ws, const to_tensor* w,
                                const to_tensor* b, int hidden_act, int out_act, int feed,
                                to_tensor X, to_tensor U_or_null, int64_t G,
                                to_tensor prime_out_or_null, to_tensor out, int64_t* symbols_or_null,
                                const to_tensor* s_out_or_null);
to_status to_set_rnn_generate_persistent(int on, int* previous_or_null);   /* 0 per step, 1 automatic, 2 wherever in range */
to_status to_rnn_generate_stats(int64_t* persistent_runs, int64_t* per_step_runs);

/* Per-sequence training of the same stacks in ONE call: `trainNetwork'` (Recurrent.hs:356-371 takes ONE sequence [(x, y)]
 * and returns the updated network) folded over a set of sequences.  For j = 0 .. n_idx-1, in order, with q = idx[j] (q = j
 * when idx is null): one to_rnn_stack_sgd step on sequence q alone -- forward over T steps from the current initial states,
 * BPTT of sum_t loss(out_t, Y_t), s -= rate_state gs and every parameter -= rate_params g, in place.  Step j + 1 sees step
 * j's parameters and initial states; as in the reference the final state of a sequence is not carried, the learned initial
 * state is.  The stack (state_act, s, ws, w, b), hidden_act, the (out_act, loss) pairs, the dtypes and the rule that initial
 * states are unbatched and contiguous are to_rnn_stack_sgd's, with its statuses.
 *   X               [N; T, i], batched and contiguous;  Y [N; T, n_L], same batch and dtype, contiguous (TO_ERR_SHAPE);
 *   idx_or_null     host int64[n_idx], entries in [0, N), repeats allowed (TO_ERR_SHAPE out of range); null: sequences
 *                   0 .. n_idx-1, n_idx <= N (TO_ERR_SHAPE).  n_idx >= 1 (TO_ERR_ARG).  The array may be reused on return;
 *   losses_or_null  contiguous [n_idx; T] of X's dtype: losses[j][t] is the loss of sequence idx[j] at step t under the
 *                   parameters step j started from.  It may overlap neither X, Y nor a parameter (TO_ERR_ARG).
 * fp32 or fp64, any N, T >= 1 and widths: never TO_ERR_UNSUPPORTED for a valid stack.  Pending operands are produced first;
 * refused during graph capture (TO_ERR_STATE); every refusal is decided before the first launch and leaves parameters,
 * states and losses untouched; blocks before returning; keeps no handle.
 * Routes.  Per sequence (A): per j, to_rnn_stack_sgd's own launches on the B = 1 views to_batch_select would give -- the
 * parameters, states and losses are BIT FOR BIT those of the caller's loop of to_rnn_stack_sgd over to_batch_select views;
 * takes every stack; launches, pool allocations and one synchronise per sequence.  Persistent (B, csrc/rnn_online.hip,
 * rnn_online_kernel): all n_idx sequences in ONE launch by ONE workgroup (nothing crosses workgroups, the kernel waits on
 * its own barriers only).  Every layer's W, W' and b and the initial states stay in LDS for the whole call -- matrices
 * k-major with an odd leading dimension, read conflict-free by the forward (a thread a column) and by the backward's W^T dz
 * and W'^T dz (a thread a k).  Only a stateful layer's own recurrence is serial in t (one barrier a step, forward and
 * backward); input projections, hidden activations, the head, the cotangents between layers and the update are spread over
 * all threads for all T steps at once.  Every sum has a fixed order (z: input part by ascending k, state part by ascending
 * k, the bias; a gradient element: ascending t; no gradient buffer exists), so the result is deterministic and n_idx = a
 * followed by n_idx = b from the first call's parameters gives the bits of the one call with a + b.  What the backward needs
 * of the forward (the tape) is in LDS where it fits beside the parameters, else in a pool buffer; the launch count depends
 * neither on n_idx nor on T and the range does not depend on T: 1..8 layers, fp32 and fp64, and the parameters, the states
 * and a few rows within 160 KiB of LDS -- fp32 64 -> 128 (stateful) -> 64 (133 KiB) and 70 -> 130 (stateful) -> 3 (107 KiB)
 * fit, fp64 70 -> 130 -> 3 (209 KiB of parameters) and fp32 64 -> 160 (stateful) -> 64 (182 KiB) do not and take route A.
 * The two routes agree to rounding, not bit for bit.  to_set_rnn_online_persistent: 0 route A; 1 automatic (default): route B
 * where its plan fits AND no layer (the input not counted) is wider than H* = 128, the largest width scanned: measured by
 * tools/rnn_online_scan.py on fp32 64 -> H (stateful) -> 10 over 256 sequences, route B was ahead of route A at H = 32, 64,
 * 96 and 128 at both T = 8 and T = 64 (profiles/rnn_online_scan.txt; logistic states, one tanh row at
 * H = 64); wider layers that still fit have NOT been measured and take route A; 2 route B wherever its plan fits.
 * Process-wide.  to_rnn_online_stats counts calls by the route that ran them. */
to_status to_rnn_stack_online_sgd(int n_layers, const int* state_act, const to_tensor* s, const to_tensor* ws, const to_tensor* w,
                                  const to_tensor* b, int hidden_act, int out_act, int loss, to_tensor X, to_tensor Y,
                                  int64_t n_idx, const int64_t* idx_or_null, double rate_state, double rate_params,
                                  to_tensor losses_or_null);
to_status to_set_rnn_online_persistent(int on, int* previous_or_null);   /* 0 per sequence, 1 automatic, 2 wherever in range */
to_status to_rnn_online_stats(int64_t* persistent_runs, int64_t* per_sequence_runs);

/* The same per-sequence training for sequences of DIFFERENT lengths -- `trainNetwork` takes a list [(x, y)] of any length,
 * and folded over a data set every sequence is one update of its own length: to_rnn_stack_online_sgd's argument list with
 * `lens` directly after the data tensors, as the ragged siblings above have it.
 *   lens  host int64[N], N = X's batch, indexed by SEQUENCE (not by position in idx); may be reused on return.  Null is
 *         TO_ERR_ARG.  Every one of the N entries must be in 1 .. T, also those of sequences idx never names: otherwise
 *         TO_ERR_SHAPE.
 * For j = 0 .. n_idx-1, in order, with q = idx[j] (q = j when idx is null): one `trainNetwork'` step on steps
 * 0 .. lens[q]-1 of sequence q alone, objective sum_{t < lens[q]} loss(out_t, Y_t), from the parameters and learned initial
 * states step j - 1 left.  The final state is not carried, the learned initial state is.
 *   Padding is never read: rows t >= lens[q] of X and Y may hold anything, NaN and Inf included, and influence no bit of
 *   any parameter, state or loss.
 *   losses_or_null  contiguous [n_idx; T]: losses[j][t] for t < lens[idx[j]] is the dense entry's quantity; exactly +0.0 at
 *                   padding.
 * Everything else is to_rnn_stack_online_sgd's, with its statuses: the stack, state_act, hidden_act, the (out_act, loss)
 * pairs, unbatched contiguous initial states, the shape rules for X / Y / idx / n_idx, the overlap rule for losses; fp32 and
 * fp64, any N, T and widths: never TO_ERR_UNSUPPORTED for a valid stack; pending operands are produced first; refused
 * during graph capture (TO_ERR_STATE); every refusal is decided before the first launch and leaves parameters, states and
 * losses untouched; blocks before returning; keeps no handle.
 * With every lens[q] == T the parameters, states and losses are the dense entry's, bit for bit, on either route.  On either
 * route n_idx = a followed by n_idx = b from the first call's result gives the bits of the one call with a + b.
 * Routes.  Per sequence (A): losses zeroed once, then per j to_rnn_stack_sgd's own launches on the rank-2 views of the
 * leading lens[q] rows of X[q] and Y[q] (contiguous: a sequence's leading rows are) and the leading lens[q] entries of
 * losses[j] -- bit for bit the caller's loop of to_rnn_stack_sgd over to_wrap views of those addresses; takes every stack.
 * Persistent (B): rnn_online_kernel with every loop over steps bounded by the sequence's own length -- one launch, one
 * workgroup, the same fixed summation orders, no wait but the kernel's own barriers; X, Y and losses keep the row stride of
 * the padded T; what a longer sequence left on the tape behind a shorter one's last step is read by nothing.  The lengths
 * reach the kernel as a device table of n_idx entries (uploaded like idx, released after the call's synchronise).  The plan
 * -- the tape's home and the pool buffer's size -- is made for the longest length the call USES, max_j lens[idx[j]]; the
 * range depends on no length.  to_set_rnn_online_persistent chooses the route exactly as for the dense entry (0 / 1 / 2, the
 * same H* = 128).  The dense entry, its launches and to_rnn_online_stats are untouched by these calls;
 * to_rnn_online_ragged_stats counts them by route.
 * Measured (tools/rnn_online_ragged_scan.py, profiles/rnn_online_ragged_scan.txt; fp32, 256 sequences padded to T = 64,
 * lengths uniform in 1..T, N T / sum lens = 2.02, logistic states, microseconds a sequence): route B 47 against route A 114
 * and the caller's loop of to_rnn_stack_sgd over to_wrap views 116 for 5 -> 7 -> 5 (2.4x ahead); 64 -> H (stateful) -> 10:
 * 57 / 135 / 137 at H = 32, 79 / 152 / 155 at 64, 111 / 187 / 190 at 96, 152 / 219 / 222 at 128 (2.4x down to 1.44x ahead).
 * Route B is ahead of route A on every scanned row, so the automatic rule H* = 128, read from equal lengths, is confirmed
 * for these rows.  Against the dense entry on the padded set (N T rows of work on ANOTHER objective -- it trains on the
 * padding; a work reference only) route B takes 1.82x (5 -> 7 -> 5) to 1.97x less, of the 2.02x the rows would give: a
 * sequence's cost follows its own length.  Where it LOSES: with every length T the ragged call is up to 5 % behind the
 * dense entry on the narrow stacks (89.4 against 85.2 for 5 -> 7 -> 5, 108.8 against 104.8 at H = 32: the lengths table and
 * the per-sequence length read) and within 1 % of it from H = 64 on -- call the dense entry for such a set.  NOT measured:
 * fp64, tanh states, other length distributions, other T. */
to_status to_rnn_stack_online_sgd_ragged(int n_layers, const int* state_act, const to_tensor* s, const to_tensor* ws,
                                         const to_tensor* w, const to_tensor* b, int hidden_act, int out_act, int loss,
                                         to_tensor X, to_tensor Y, const int64_t* lens, int64_t n_idx,
                                         const int64_t* idx_or_null, double rate_state, double rate_params,
                                         to_tensor losses_or_null);
to_status to_rnn_online_ragged_stats(int64_t* persistent_runs, int64_t* per_sequence_runs);

/* `induceNetwork` (FeedForward.hs:150-164) of the same ffLayer stacks, iterated: gradient descent on the INPUT with the
 * parameters fixed (app/MNIST.hs:357-365 runs 5000 such steps in a row), for every row of the hidden batch, in ONE call:
 *   x_0 = x[r];   g_k = d/dx loss(net(x_k), y[r]);   x_{k+1} = x_k - rate * g_k,   k = 0 .. iters-1
 *   out[r] = x_iters     gx[r] = g_{iters-1}     losses[r, k] = loss(net(x_k), y[r])   (the loss BEFORE step k+1)
 * hidden_act TO_ACT_LOGISTIC or TO_ACT_TANH; (out_act, loss) (TO_ACT_SOFTMAX, TO_LOSS_CROSS_ENTROPY) or (TO_ACT_LOGISTIC,
 * TO_LOSS_SQUARED_ERROR), anything else TO_ERR_UNSUPPORTED with nothing written; the losses are to_fflayer_stack_grad's.
 * Targets are arbitrary vectors, not only one-hot.  No clamping of x: the reference has none.
 *   x               [B; i0] or unbatched [i0] (one row);
 *   y               [B; n_L] of x's batch, or unbatched [n_L]: one target for every row;
 *   out             caller-allocated, contiguous, of x's shape, batch and dtype; MAY BE x ITSELF (in place);
 *   gx_or_null      like out: the gradient of the last iteration -- with iters = 1 it is `head' (netGrad ...)`, the input
 *                   cotangent that to_fflayer_stack_grad does not return.  Needs iters >= 1 (TO_ERR_ARG);
 *   losses_or_null  contiguous [B; iters] (unbatched [iters] for an unbatched x).
 * iters >= 0; iters == 0 copies x to out bit for bit and touches nothing else.  fp32 or fp64, any B, any widths, one layer
 * or more: never TO_ERR_UNSUPPORTED for a valid stack and pair.  Parameters and y are only read; pending operands are
 * produced first; refused during graph capture (TO_ERR_STATE); blocks before it returns; keeps no handle.  A refused or
 * failed call leaves out, gx and losses untouched.
 * Routes.  Per iteration (A): one GEMM a layer forward (bias + activation in its epilogue), the loss head, the cotangents
 * back, and the last contraction with the step in its epilogue; takes every stack, launches grow with iters.  Persistent
 * (B, csrc/induce_seq.hip): all iterations of all rows in ONE launch, the parameters in LDS, layer 1 split by columns over
 * G <= 32 workgroups of one XCD that exchange o1 partial sums an iteration (G = 1: no exchange).  Its range: 1..6 layers,
 * n_L <= 64, the smallest G whose workgroups fit 160 KiB of LDS -- fp32 784-300-100-10 at G = 32, fp64 784-300-100-10 does
 * not fit (route A) -- and, for G > 1, a device on which the workgroups of the group share an XCD (probed; elsewhere the
 * call takes route A).  A wait of the persistent kernel that times out (TOPS_ONLINE_TIMEOUT_S, 2 s) is TO_ERR_HIP naming the
 * iteration; there is no retry and no silent fall-back.  On either route a row's bits depend neither on B nor on the row's
 * place in the batch, and iters = a followed by iters = b on the result equals iters = a + b bit for bit.
 * to_set_induce_persistent: 0 route A; 1 automatic (default): route B where it is known to be ahead -- until the scan of
 * DESIGN.md section 3.3 has been run on a device that is a plan of one workgroup a row (G = 1) with B <= 256, route A
 * otherwise; 2 route B wherever its plan fits, A otherwise (the rule does not look at hidden_act and has not been measured
 * for tanh).  Process-wide.  to_induce_stats counts calls (iters >= 1) by
 * the route that ran. */
to_status to_fflayer_stack_induce(int n_layers, const to_tensor* w, const to_tensor* b, int hidden_act, int out_act,
                                  int loss, to_tensor x, to_tensor y, double rate, int64_t iters, to_tensor out,
                                  to_tensor gx_or_null, to_tensor losses_or_null);
to_status to_set_induce_persistent(int on, int* previous_or_null);
to_status to_induce_stats(int64_t* persistent_runs, int64_t* per_iteration_runs);

/* Debug: the plan of one of the two persistent kernels whose workgroups share layer 1 -- to_fflayer_stack_online_sgd's
 * (csrc/online_sgd.hip: layer 1 split by ROWS) or route B of to_fflayer_stack_induce (csrc/induce_seq.hip: by COLUMNS) --
 * for the stack dims[0 .. n_layers] = i0, o1 .. oL, as the entry itself would get it, without running the kernel.  B and
 * iters are read for TO_PERSIST_INDUCE only.  *exists: the kernel takes the stack (else every other output but
 * *placement_ok is 0); *G: workgroups that share a sample / a row; *slice: rows (online) or columns (induce) of layer 1
 * per workgroup; *last_slice: those of workgroup G - 1; *lds_bytes: dynamic LDS per workgroup; *grid: workgroups launched
 * (8 G where G > 1 and for every online plan; min(B, 256) for an induce plan with G = 1); *placement_ok: whether workgroups
 * b, b + 8, .. of a grid share an XCD on this device (probed once a process), which every online plan and every induce plan
 * with G > 1 needs.  n_layers 1..7 (a stack deeper than a kernel's range has no plan).  TO_ERR_STATE before to_init. */
enum { TO_PERSIST_ONLINE_SGD = 0, TO_PERSIST_INDUCE = 1 };
to_status to_persist_plan_query(int kernel, int dtype, int n_layers, const int64_t* dims, int64_t B, int64_t iters,
                                int* exists, int* G, int* slice, int* last_slice, int64_t* lds_bytes, int64_t* grid,
                                int* placement_ok);

/* ---- measurement ---------------------------------------------------------------------- */
/* Average duration (ms) of kernels enqueued between the two calls, measured with
 * HIP events on the library's stream. */
to_status to_timer_start(void);
to_status to_timer_stop(float* ms);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* TENSOROPS_HIP_H */
