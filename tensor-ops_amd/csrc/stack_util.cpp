#include "stack_util.hpp"

#include "api_util.hpp"

namespace to {

int stack_hidden_act_check(int hidden_act, const char* prefix) {
  TO_CHECK(hidden_act == TO_ACT_LOGISTIC || hidden_act == TO_ACT_TANH, TO_ERR_UNSUPPORTED,
           std::string(prefix) + "hidden activation must be logistic or tanh");
  return hidden_act == TO_ACT_TANH ? ACT_KIND_TANH : ACT_KIND_LOGISTIC;
}

int stack_loss_head(int out_act, int loss, const std::string& prefix) {
  if (out_act == TO_ACT_SOFTMAX && loss == TO_LOSS_CROSS_ENTROPY) return 1;
  if (out_act == TO_ACT_LOGISTIC && loss == TO_LOSS_SQUARED_ERROR) return 2;
  fail(TO_ERR_UNSUPPORTED, prefix + "(softmax, crossEntropy) or (logistic, squaredError) only");
}

int64_t stack_params_check(int n_layers, const to_tensor* w, const to_tensor* b, const to_tensor* gw, const to_tensor* gb,
                           int dt, int64_t fan_in) {
  for (int l = 0; l < n_layers; ++l) {
    NONNULL(w[l]); NONNULL(b[l]);
    if (gw) { NONNULL(gw[l]); NONNULL(gb[l]); }
    TO_CHECK(w[l]->dtype == dt && b[l]->dtype == dt && (!gw || (gw[l]->dtype == dt && gb[l]->dtype == dt)), TO_ERR_ARG,
             gw ? "parameters, gradients and data must share one dtype" : "parameters and data must share one dtype");
    TO_CHECK(w[l]->rank == 2 && w[l]->batch == 0 && w[l]->dims[1] == fan_in && w[l]->contiguous(),
             TO_ERR_SHAPE, "layer " + std::to_string(l) + ": W has shape " + shape_str(w[l]));
    TO_CHECK(b[l]->rank == 1 && b[l]->batch == 0 && b[l]->dims[0] == w[l]->dims[0] && b[l]->contiguous(),
             TO_ERR_SHAPE, "layer " + std::to_string(l) + ": b has shape " + shape_str(b[l]));
    if (gw)
      TO_CHECK(same_shape(gw[l], w[l]) && gw[l]->contiguous() && same_shape(gb[l], b[l]) && gb[l]->contiguous(),
               TO_ERR_SHAPE, "gradient destinations must match the parameters");
    fan_in = w[l]->dims[0];
  }
  return fan_in;
}

bool stack_overlap(to_tensor s, to_tensor t) {
  if (!s || !t || !s->ptr || !t->ptr) return false;
  auto end = [](to_tensor u) {
    int64_t last = u->batch > 1 ? (u->batch - 1) * u->bstride : 0;
    for (int d = 0; d < u->rank; ++d) last += (u->dims[d] - 1) * u->strides[d];
    return static_cast<const char*>(u->ptr) + (last + 1) * (int64_t)u->esize();
  };
  return static_cast<const char*>(s->ptr) < end(t) && static_cast<const char*>(t->ptr) < end(s);
}

void ew2(int dt, int kind, void* out, const void* x0, const void* x1, int64_t n) {
  EwArgs a{};
  a.dtype = dt;
  a.kind = kind;
  a.n = x1 ? 2 : 1;
  a.x[0] = x0;
  a.x[1] = x1;
  a.period[0] = a.period[1] = n;
  a.coef[0] = a.coef[1] = 1.0;
  a.out = out;
  a.total = n;
  launch_ewise(a, S());
}

GemmProblem row_gemm(int dt, const void* A, int64_t a_sm, int64_t a_sk, const void* B, int64_t b_sk, int64_t b_sn, void* C,
                     int64_t M, int64_t N, int64_t K) {
  GemmProblem p{};
  p.dtype = dt;
  p.A = A; p.B = B; p.C = C;
  p.M = M; p.N = N; p.K = K;
  p.a_sm = a_sm; p.a_sk = a_sk; p.b_sk = b_sk; p.b_sn = b_sn; p.c_sm = N;
  p.batch = 1;
  p.alpha = 1.0; p.beta = 0.0;
  return p;
}

void gemm_with_epilogue(GemmProblem p) {
  if (gemm_epilogue_ok(p)) return run_gemm_small_first(p);
  const int act = p.act, dact_kind = p.dact_kind;
  const void* dact = p.dact;
  if (p.bias) {  // C = bias rows, then C += A B
    TO_CHECK(p.beta == 0.0, TO_ERR_STATE, "internal: bias with an addend");
    launch_bcast_axis(p.dtype, p.bias, p.C, 1, p.M, p.N, 0, S());
    p.beta = 1.0;
    p.Cin = p.C;
  }
  TO_CHECK(!(act && dact), TO_ERR_STATE, "internal: act and dact in one epilogue");
  p.bias = nullptr; p.act = 0; p.dact = nullptr; p.dact_kind = 0;
  run_gemm(p);
  if (act) ew2(p.dtype, act == 2 ? EW_TANH : EW_LOGISTIC, p.C, p.C, nullptr, p.M * p.N);
  else if (dact) ew2(p.dtype, dact_kind ? EW_MUL_1MH2 : EW_MUL_H1MH, p.C, p.C, dact, p.M * p.N);
}

void stack_layer_forward(int dt, to_tensor W, to_tensor bias, int act_kind, const void* A, int64_t a_sm, void* C, int64_t B) {
  GemmProblem p = row_gemm(dt, A, a_sm, 1, W->ptr, 1, W->dims[1], C, B, W->dims[0], W->dims[1]);
  p.bias = bias->ptr;
  p.act = act_kind + 1;
  if (gemm_epilogue_ok(p)) return run_gemm_small_first(p);
  p.bias = nullptr;   // (the tiled fp64 kernel: alpha / beta only)
  p.act = 0;
  run_gemm(p);
  launch_bias_act_rows(dt, C, bias->ptr, B, W->dims[0], act_kind, S());
}

void run_online_sgd(int dt, int n_layers, const int64_t* dims, void* const* W, void* const* b, to_tensor X, to_tensor Y,
                    const int64_t* idx_host, int64_t n_idx, double rate, int head, int hidden_kind) {
  Holder order;
  const long long* idx_dev = nullptr;
  if (idx_host) {
    const int64_t nl = (n_idx * 8 + 3) / 4;
    order.t = new_tensor(1, &nl, 0);
    host_to_device(order.t->ptr, idx_host, (size_t)n_idx * sizeof(int64_t), S());
    idx_dev = static_cast<const long long*>(order.t->ptr);
  }
  online_sgd_reset_status();
  launch_online_sgd(dt, n_layers, dims, W, b, X->ptr, Y->ptr, idx_dev, n_idx, rate, head, hidden_kind, S());
  TO_HIP(hipStreamSynchronize(S()));  // the order buffer goes back to the pool; the watchdog's verdict is read
  TO_CHECK(online_sgd_status() == 0, TO_ERR_HIP,
           "online SGD kernel: a workgroup barrier timed out at sample " + std::to_string(online_sgd_status() - 1) +
               " (the write-back is all-or-nothing: commit or abort is ONE word decided by compare-and-swap and obeyed by every workgroup; this run aborted, the parameters are unchanged)");
}

}  // namespace to
