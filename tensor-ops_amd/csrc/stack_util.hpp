// What the one-call stack entries (stack_ff.cpp, stack_rnn.cpp) and to_graph_online_sgd (api.cpp) share.  Every entry runs
// in the same order: validate, ensure the operands, claim the destinations, launch.  (gemm_small_takes, which they ask before a
// step's launches, lives with the other routing predicates in gemm_route.hpp.)
#pragma once
#include "ops.hpp"

namespace to {

// Hidden layers: logistic or tanh.  Returns the activation numbered as the kernels number it (ACT_KIND_*:
// GemmProblem::dact_kind / tail_kind, the persistent kernels' template parameter; GemmProblem::act is this + 1).
int stack_hidden_act_check(int hidden_act, const char* prefix = "fused path: ");
// The (output activation, loss) pair as the kernels' head number: 1 = (softmax, crossEntropy), 2 = (logistic, squaredError).
int stack_loss_head(int out_act, int loss, const std::string& prefix);
inline int loss_grad_rows_kind(int head) { return head - 1; }  // launch_loss_grad_rows numbers the same pairs 0 / 1
// Every layer's W [n_l, n_{l-1}] and b [n_l]: unbatched, contiguous, of the data's dtype, chained from `fan_in`; gradient
// destinations (gw / gb null: none) of the parameters' shapes.  Returns n_L.
int64_t stack_params_check(int n_layers, const to_tensor* w, const to_tensor* b, const to_tensor* gw, const to_tensor* gb,
                           int dt, int64_t fan_in);

// a destination: its storage exists, recorded readers of the old value have run, new identity
inline void claim(to_tensor t) { ensure(t); before_write(t); t->id = fresh_id(); }
inline void* at(const void* p, int64_t elems, int64_t es) {
  return static_cast<char*>(const_cast<void*>(p)) + elems * es;
}
// Do the extents of s and t (first to last addressed byte) share a byte?  Null handles and handles without storage yet
// share none.  (`overlaps` of lazy.cpp is another predicate: it treats zero-extent handles differently.)
bool stack_overlap(to_tensor s, to_tensor t);
// t's rows with unit element stride: t itself, or a packed copy (held by h) of a strided vector view.  Null for null.
inline to_tensor unit_stride_rows(to_tensor t, Holder& h) {
  if (t && t->dims[0] > 1 && t->strides[0] != 1) h.t = contiguous(t);
  return h.t ? h.t : t;
}
// out[i] = kind(x0[i]) or kind(x0[i], x1[i]) (EwKind; x1 null: one input), i < n
void ew2(int dt, int kind, void* out, const void* x0, const void* x1, int64_t n);

// C[M, N] (contiguous) = A[M, K] (rows a_sm apart) . Bop where Bop(k, n) = B[k * b_sk + n * b_sn]
GemmProblem row_gemm(int dt, const void* A, int64_t a_sm, int64_t a_sk, const void* B, int64_t b_sk, int64_t b_sn, void* C,
                     int64_t M, int64_t N, int64_t K);
// C = A . B(op) with the epilogue of p (bias, act = logistic / tanh, dact = h (1 - h) / 1 - h h by dact_kind, beta * Cin); a
// kernel without one gets the plain product and the epilogue as separate launches.  C is contiguous [M, N].
void gemm_with_epilogue(GemmProblem p);
// C[B, n] = act(A W^T + b), one layer of a stack over B rows (act_kind: ACT_KIND_*): one GEMM with the epilogue where the
// kernel carries one, else the plain product and one elementwise launch
void stack_layer_forward(int dt, to_tensor W, to_tensor bias, int act_kind, const void* A, int64_t a_sm, void* C, int64_t B);

// The persistent online-SGD kernel over n_idx > 0 samples of X / Y (idx_host null: rows 0 .. n_idx-1), then a stream
// synchronise; throws TO_ERR_HIP when its watchdog aborted the run (the parameters are then unchanged).
void run_online_sgd(int dt, int n_layers, const int64_t* dims, void* const* W, void* const* b, to_tensor X, to_tensor Y,
                    const int64_t* idx_host, int64_t n_idx, double rate, int head, int hidden_kind);

}  // namespace to
