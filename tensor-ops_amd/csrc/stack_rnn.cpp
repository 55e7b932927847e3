// ---- recurrent stacks: `runNetwork` / `netGrad` / `trainNetwork'` of Recurrent.hs as one call -------------------------
// Layer l is `fullyConnected` (Recurrent.hs:91-119; z = W x + W' s + b, new state state_act[l](z) -- logistic or tanh, each
// layer its own --, output z through the layer's `*~ act`, hidden_act) or a stateless ffLayer (:126-138).  Internally everything is TIME-MAJOR, row r = t * B + b, so that every
// time-independent piece is ONE contraction over all B*T rows: the input projections (bias in the epilogue), the head,
// the weight gradients dZ^T X and dZ^T S_prev (+ the bias row sums) and the input cotangents dZ W (hidden_act' of the layer
// below in the epilogue).  A stateful layer's states live in St [T+1][B][n] with block 0 = the initial states: S_prev and
// S are the two offset views St[0..T) and St[1..T] of one buffer.  What is left is each stateful layer's recurrence:
// persistent (rnn_seq.hip, one launch per layer and direction for all T steps) or per step (one GEMM with the addend,
// plus one elementwise launch).  The caller's [B; T, .] rows are moved to and from time-major by one strided copy each.
#include "api_util.hpp"
#include "stack_util.hpp"

using namespace to;

extern "C" {

static int g_rnn_persistent = 1;                          // to_set_rnn_persistent: 0 per step, 1 auto, 2 wherever in range
static int64_t g_rnn_persistent_runs = 0, g_rnn_stepwise_runs = 0;

// Does the persistent kernel take a layer of width H over a batch of B sequences?  The automatic rule is the threshold
// measured by tools/rnn_scan.py (profiles/r07_rnn_scan.txt): the kernel wins while W' sits in its
// LDS (H = 64: 2-4x ahead of the per-step route at every B and T) and loses once every step streams W' from L2 into ONE
// workgroup (H = 256 / 512: up to 4.4x behind), so automatic = persistent exactly when the plan holds W' in LDS.
static bool rnn_persistent_for(int dt, int64_t H, int64_t B, RnnSeqPlan* plan) {
  if (g_rnn_persistent == 0 || !rnn_seq_plan(dt, H, B, plan)) return false;
  return g_rnn_persistent == 2 || plan->m_lds;
}

enum class RnnMode { Run, Grad, Sgd };
struct RnnStackArgs {  // what the three entries hand to rnn_stack_impl; each fills what it has
  RnnMode mode;
  int n_layers;
  const int* state_act;
  const to_tensor *s, *ws, *w, *b;
  int hidden_act, out_act;
  to_tensor X;
  int loss = -1;  // from here on: null / unset unless the entry has it
  to_tensor Y = nullptr, out = nullptr, gx = nullptr, losses = nullptr;
  const to_tensor *s_out = nullptr, *gs = nullptr, *gws = nullptr, *gw = nullptr, *gb = nullptr;
  double rate_state = 0.0, rate_params = 0.0;
};

static void rnn_stack_impl(const RnnStackArgs& a) {
  const bool run = a.mode == RnnMode::Run, grad = a.mode == RnnMode::Grad, sgd = a.mode == RnnMode::Sgd;
  const int n_layers = a.n_layers, hidden_act = a.hidden_act, out_act = a.out_act;
  const int* state_act = a.state_act;
  const to_tensor *s = a.s, *ws = a.ws, *w = a.w, *b = a.b, *s_out = a.s_out, *gs = a.gs, *gws = a.gws, *gw = a.gw, *gb = a.gb;
  const to_tensor X = a.X, Y = a.Y, out = a.out, gx = a.gx, losses = a.losses;
  const char* fn = run ? "to_rnn_stack_run" : grad ? "to_rnn_stack_grad" : "to_rnn_stack_sgd";
  const std::string F = std::string(fn) + ": ";
  require_init();
  no_capture(fn);
  NONNULL(state_act); NONNULL(s); NONNULL(ws); NONNULL(w); NONNULL(b); NONNULL(X);
  TO_CHECK(n_layers >= 1, TO_ERR_ARG, F + "need at least one layer");
  for (int l = 0; l < n_layers; ++l)
    TO_CHECK(state_act[l] == TO_ACT_LOGISTIC || state_act[l] == TO_ACT_TANH || state_act[l] == TO_RNN_STATELESS,
             TO_ERR_UNSUPPORTED,
             F + "layer " + std::to_string(l) + ": the state activation must be logistic or tanh (or TO_RNN_STATELESS)");
  const int hk = stack_hidden_act_check(hidden_act);
  auto state_kind = [&](int l) { return state_act[l] == TO_ACT_TANH ? ACT_KIND_TANH : ACT_KIND_LOGISTIC; };
  int head = 0;
  if (run)
    TO_CHECK(out_act == TO_ACT_SOFTMAX || out_act == TO_ACT_LOGISTIC, TO_ERR_UNSUPPORTED,
             F + "the output activation must be softmax or logistic");
  else
    head = stack_loss_head(out_act, a.loss, F);
  const int dt = X->dtype;
  TO_CHECK(X->rank == 2 && X->dims[0] >= 1 && X->dims[1] >= 1, TO_ERR_SHAPE,
           F + "X must be [B; T, i] (or [T, i]), got " + shape_str(X));
  const int64_t T = X->dims[0], B = X->batch > 0 ? X->batch : 1;
  if (grad) { NONNULL(gs); NONNULL(gws); NONNULL(gw); NONNULL(gb); }
  const int64_t nL = stack_params_check(n_layers, w, b, gw, gb, dt, X->dims[1]);
  auto seq_like = [&](to_tensor t, int64_t n, const char* what) {  // [B; T, n] of X's batch and dtype, contiguous
    TO_CHECK(t->dtype == dt, TO_ERR_ARG, F + what + " and X have different dtypes");
    TO_CHECK(t->rank == 2 && t->dims[0] == T && t->dims[1] == n && t->batch == X->batch, TO_ERR_SHAPE,
             F + what + " must be [B; " + std::to_string(T) + ", " + std::to_string(n) + "] of X's batch, got " + shape_str(t));
  };
  for (int l = 0; l < n_layers; ++l) {
    const int64_t n = w[l]->dims[0];
    const std::string L = F + "layer " + std::to_string(l) + ": ";
    if (state_act[l] == TO_RNN_STATELESS) {
      TO_CHECK(!s[l] && !ws[l], TO_ERR_ARG, L + "a stateless layer has no state and no W'");
      if (grad) TO_CHECK(!gs[l] && !gws[l], TO_ERR_ARG, L + "a stateless layer has no state gradients");
      if (run && s_out) TO_CHECK(!s_out[l], TO_ERR_ARG, L + "a stateless layer has no final state");
      continue;
    }
    NONNULL(s[l]); NONNULL(ws[l]);
    TO_CHECK(s[l]->dtype == dt && ws[l]->dtype == dt, TO_ERR_ARG, L + "states, parameters and data must share one dtype");
    TO_CHECK(ws[l]->rank == 2 && ws[l]->batch == 0 && ws[l]->dims[0] == n && ws[l]->dims[1] == n && ws[l]->contiguous(),
             TO_ERR_SHAPE, L + "W' has shape " + shape_str(ws[l]));
    TO_CHECK(s[l]->rank == 1 && s[l]->dims[0] == n, TO_ERR_SHAPE, L + "s has shape " + shape_str(s[l]));
    if (run)
      TO_CHECK(s[l]->batch == 0 || s[l]->batch == X->batch, TO_ERR_SHAPE,
               L + "s must be unbatched or of X's batch, got " + shape_str(s[l]));
    else
      TO_CHECK(s[l]->batch == 0 && s[l]->contiguous(), TO_ERR_SHAPE,
               L + "the initial state of grad / sgd must be unbatched and contiguous, got " + shape_str(s[l]));
    if (grad) {
      NONNULL(gs[l]); NONNULL(gws[l]);
      TO_CHECK(gs[l]->dtype == dt && gws[l]->dtype == dt, TO_ERR_ARG, L + "gradients and data must share one dtype");
      TO_CHECK(same_shape(gs[l], s[l]) && gs[l]->batch == 0 && gs[l]->contiguous() && same_shape(gws[l], ws[l]) &&
                   gws[l]->contiguous(), TO_ERR_SHAPE, L + "gradient destinations must match the state and W'");
    }
    if (run && s_out && s_out[l]) {
      TO_CHECK(s_out[l]->dtype == dt, TO_ERR_ARG, L + "s_out and X have different dtypes");
      TO_CHECK(s_out[l]->rank == 1 && s_out[l]->dims[0] == n && s_out[l]->batch == X->batch && s_out[l]->contiguous(),
               TO_ERR_SHAPE, L + "s_out must be a contiguous [B; n] of X's batch, got " + shape_str(s_out[l]));
    }
  }
  if (run) {
    NONNULL(out);
    seq_like(out, nL, "out");
    TO_CHECK(out->contiguous(), TO_ERR_ARG, F + "out must be contiguous");
  } else {
    NONNULL(Y);
    seq_like(Y, nL, "Y");
    if (gx) { seq_like(gx, X->dims[1], "gx"); TO_CHECK(gx->contiguous(), TO_ERR_ARG, F + "gx must be contiguous"); }
    if (losses) {
      TO_CHECK(losses->dtype == dt, TO_ERR_ARG, F + "losses and X have different dtypes");
      TO_CHECK(losses->rank == 1 && losses->dims[0] == T && losses->batch == X->batch && losses->contiguous(),
               TO_ERR_SHAPE, F + "losses must be a contiguous [B; T] of X's batch, got " + shape_str(losses));
    }
  }
  TO_CHECK(T * B <= 2147483647LL, TO_ERR_SHAPE, F + "more than 2^31-1 rows");

  // ---- operands produced; destinations claimed -------------------------------------------------------------------
  ensure(X);
  if (Y) ensure(Y);
  for (int l = 0; l < n_layers; ++l) {
    ensure(w[l]); ensure(b[l]);
    if (s[l]) { ensure(s[l]); ensure(ws[l]); }
  }
  if (out) claim(out);
  if (s_out) for (int l = 0; l < n_layers; ++l) if (s_out[l]) claim(s_out[l]);
  if (gx) claim(gx);
  if (losses) claim(losses);
  if (grad)
    for (int l = 0; l < n_layers; ++l) {
      claim(gw[l]); claim(gb[l]);
      if (gs[l]) { claim(gs[l]); claim(gws[l]); }
    }

  const int64_t rows = T * B;
  const int64_t es = dt == TO_F64 ? 8 : 4;
  // [B; T, n] (strides of t) -> time-major [T][B][n]
  auto to_time_major = [&](to_tensor t, Holder& h) -> const void* {
    if (B == 1 && t->contiguous()) return t->ptr;
    const int64_t n = t->dims[1];
    const int64_t d3[3] = {T, B, n}, s3[3] = {t->strides[0], t->batch > 0 ? t->bstride : 0, t->strides[1]};
    const int64_t dims2[2] = {T * B, n};
    h.t = new_tensor(2, dims2, 0, dt);
    launch_copy_strided(dt, t->ptr, h.t->ptr, 3, d3, s3, S());
    return h.t->ptr;
  };
  // time-major [T][B][n] -> the caller's contiguous [B; T, n]
  auto from_time_major = [&](const void* src, to_tensor dst, int64_t n) {
    if (src == dst->ptr) return;
    const int64_t d3[3] = {B, T, n}, s3[3] = {n, B * n, 1};
    launch_copy_strided(dt, src, dst->ptr, 3, d3, s3, S());
  };
  // scratch of `rows` x n, or the caller's own buffer when it is time-major already (B == 1)
  auto scratch_or = [&](to_tensor dst, int64_t n, Holder& h) -> void* {
    if (dst && B == 1) return dst->ptr;
    const int64_t d2[2] = {rows, n};
    h.t = new_tensor(2, d2, 0, dt);
    return h.t->ptr;
  };
  Holder xh, yh;
  const void* Xt = to_time_major(X, xh);
  const void* Yt = !run ? to_time_major(Y, yh) : nullptr;

  // ---- forward -------------------------------------------------------------------------------------------------------
  std::vector<Holder> Z(n_layers), St(n_layers), WT(n_layers), Ah(n_layers);
  std::vector<const void*> outp(n_layers, nullptr);   // what the layer above reads: hidden_act(z_l), all rows
  std::vector<RnnSeqPlan> plan(n_layers);
  std::vector<char> persist(n_layers, 0);
  bool any_state = false, all_persistent = true;
  const void* prev = Xt;
  int64_t prev_n = X->dims[1];
  const void* no_bias_for_head = nullptr;  // run, stateless last layer: the head launch adds b_L
  for (int l = 0; l < n_layers; ++l) {
    const int64_t n = w[l]->dims[0];
    const bool last = l + 1 == n_layers, stateful = state_act[l] != TO_RNN_STATELESS;
    const int64_t d2[2] = {rows, n};
    Z[l].t = new_tensor(2, d2, 0, dt);
    // the input projection (stateless hidden layer: its activation) over all rows
    GemmProblem p = row_gemm(dt, prev, prev_n, 1, w[l]->ptr, 1, prev_n, Z[l].t->ptr, rows, n, prev_n);
    p.bias = b[l]->ptr;
    if (!stateful && !last) p.act = hk + 1;
    if (last && !stateful && run) { p.bias = nullptr; no_bias_for_head = b[l]->ptr; }
    gemm_with_epilogue(p);
    if (stateful) {
      any_state = true;
      const int64_t d3[2] = {(T + 1) * B, n};
      St[l].t = new_tensor(2, d3, 0, dt);
      void* st = St[l].t->ptr;
      if (s[l]->batch == 0) {
        launch_bcast_axis(dt, s[l]->ptr, st, 1, B, n, 0, S());
      } else {
        const int64_t dd[2] = {B, n}, ss[2] = {s[l]->bstride, s[l]->strides[0]};
        launch_copy_strided(dt, s[l]->ptr, st, 2, dd, ss, S());
      }
      persist[l] = rnn_persistent_for(dt, n, B, &plan[l]);
      all_persistent = all_persistent && persist[l];
      void* z = Z[l].t->ptr;
      if (persist[l]) {
        const int64_t dd[2] = {n, n}, ss[2] = {1, n};  // W'^T: M[k][j] = W'[j][k]
        WT[l].t = new_tensor(2, dd, 0, dt);
        launch_copy_strided(dt, ws[l]->ptr, WT[l].t->ptr, 2, dd, ss, S());
        launch_rnn_seq(dt, false, plan[l], WT[l].t->ptr, z, st, B, T, n, state_kind(l), S());
      } else {
        for (int64_t t = 0; t < T; ++t) {  // z_t = P_t + s_{t-1} W'^T (in place), s_t = state_act(z_t)
          GemmProblem q = row_gemm(dt, at(st, t * B * n, es), n, 1, ws[l]->ptr, 1, n, at(z, t * B * n, es), B, n, n);
          q.beta = 1.0;
          q.Cin = q.C;
          gemm_with_epilogue(q);
          ew2(dt, state_kind(l) == ACT_KIND_TANH ? EW_TANH : EW_LOGISTIC, at(st, (t + 1) * B * n, es), at(z, t * B * n, es), nullptr,
              B * n);
        }
      }
    }
    // what the layer above reads: a hidden stateful layer's output hidden_act(z) IS its state when the two activations
    // are the same function; otherwise it is one more elementwise pass over all rows of z
    if (stateful && !last && state_kind(l) == hk) {
      prev = at(St[l].t->ptr, B * n, es);
    } else if (stateful && !last) {
      Ah[l].t = new_tensor(2, d2, 0, dt);
      ew2(dt, hk == ACT_KIND_TANH ? EW_TANH : EW_LOGISTIC, Ah[l].t->ptr, Z[l].t->ptr, nullptr, rows * n);
      prev = Ah[l].t->ptr;
    } else {
      prev = Z[l].t->ptr;
    }
    outp[l] = prev;
    prev_n = n;
  }
  if (any_state) (all_persistent ? g_rnn_persistent_runs : g_rnn_stepwise_runs)++;
  const int L = n_layers - 1;
  if (run) {
    if (s_out)
      for (int l = 0; l < n_layers; ++l)
        if (s_out[l])
          TO_HIP(hipMemcpyAsync(s_out[l]->ptr, at(St[l].t->ptr, T * B * w[l]->dims[0], es), (size_t)(B * w[l]->dims[0] * es),
                                hipMemcpyDeviceToDevice, S()));
    Holder oh, zb;
    const void* bias = no_bias_for_head;
    if (!bias) {
      zb.t = new_tensor(1, &nL, 0, dt);
      launch_fill(dt, zb.t->ptr, nL, 0.0, S());
      bias = zb.t->ptr;
    }
    TO_CHECK(nL <= 2147483647LL, TO_ERR_SHAPE, F + "output layer too wide");
    void* ot = scratch_or(out, nL, oh);
    launch_infer_rows(dt, Z[L].t->ptr, rows, bias, (int)nL, out_act == TO_ACT_SOFTMAX, ot, nullptr, 0, nullptr, nullptr,
                      S());
    from_time_major(ot, out, nL);
    TO_HIP(hipStreamSynchronize(S()));
    return;
  }

  // ---- backward ------------------------------------------------------------------------------------------------------
  // gradient destinations: the caller's (grad) or scratch (sgd: applied at the end, so that a failure updates nothing)
  std::vector<Holder> tg(4 * n_layers);
  std::vector<void*> g_s(n_layers, nullptr), g_ws(n_layers, nullptr), g_w(n_layers), g_b(n_layers);
  for (int l = 0; l < n_layers; ++l) {
    auto dest = [&](const to_tensor* given, to_tensor like, Holder& h) -> void* {
      if (grad) return given[l]->ptr;
      h.t = new_tensor(like->rank, like->dims, 0, dt);
      return h.t->ptr;
    };
    g_w[l] = dest(gw, w[l], tg[4 * l]);
    g_b[l] = dest(gb, b[l], tg[4 * l + 1]);
    if (state_act[l] != TO_RNN_STATELESS) {
      g_s[l] = dest(gs, s[l], tg[4 * l + 2]);
      g_ws[l] = dest(gws, ws[l], tg[4 * l + 3]);
    }
  }
  Holder dzL, lh;
  {
    const int64_t d2[2] = {rows, nL};
    dzL.t = new_tensor(2, d2, 0, dt);
  }
  void* lt = nullptr;
  if (losses) {
    if (B == 1) lt = losses->ptr;
    else { const int64_t nr = rows; lh.t = new_tensor(1, &nr, 0, dt); lt = lh.t->ptr; }
  }
  launch_loss_grad_rows(dt, Z[L].t->ptr, Yt, dzL.t->ptr, lt, rows, nL, loss_grad_rows_kind(head), S());
  if (losses && lt != losses->ptr) {  // [T][B] -> [B][T]
    const int64_t dd[2] = {B, T}, ss[2] = {1, B};
    launch_copy_strided(dt, lt, losses->ptr, 2, dd, ss, S());
  }
  Holder dz_cur(dzL.take()), gxh;
  for (int l = L; l >= 0; --l) {
    const int64_t n = w[l]->dims[0], m = w[l]->dims[1];
    const bool stateful = state_act[l] != TO_RNN_STATELESS;
    void* dz = dz_cur.t->ptr;
    if (stateful) {  // dz_t = G_t + (dz_{t+1} W') (.) state_act'(s_t), in place over G
      void* st = St[l].t->ptr;
      if (persist[l]) {
        launch_rnn_seq(dt, true, plan[l], ws[l]->ptr, dz, st, B, T, n, state_kind(l), S());
      } else {  // per step: D = (dz_{t+1} W') (.) state_act'(s_t), then dz_t += D
        const int64_t d2[2] = {B, n};
        Holder dtmp(new_tensor(2, d2, 0, dt));
        for (int64_t t = T - 2; t >= 0; --t) {
          GemmProblem q = row_gemm(dt, at(dz, (t + 1) * B * n, es), n, 1, ws[l]->ptr, n, 1, dtmp.t->ptr, B, n, n);
          q.dact = at(st, (t + 1) * B * n, es);
          q.dact_kind = state_kind(l);
          gemm_with_epilogue(q);
          ew2(dt, EW_AFFINE, at(dz, t * B * n, es), at(dz, t * B * n, es), dtmp.t->ptr, B * n);
        }
      }
      // gW' = dZ^T S_prev ; gs = (sum_b dz_0[b]) W'
      run_gemm(row_gemm(dt, dz, 1, n, st, n, 1, g_ws[l], n, n, rows));
      Holder dsum(new_tensor(1, &n, 0, dt));
      launch_sum_axis(dt, dz, dsum.t->ptr, 1, B, n, 0, n, 1, S());
      run_gemm(row_gemm(dt, dsum.t->ptr, n, 1, ws[l]->ptr, n, 1, g_s[l], 1, n, n));
    }
    // gW = dZ^T A_in (+ gb = the row sums of dZ)
    const void* a_in = l > 0 ? outp[l - 1] : Xt;
    GemmProblem p = row_gemm(dt, dz, 1, n, a_in, m, 1, g_w[l], n, m, rows);
    p.rowsum = g_b[l];
    if (gemm_small_route(p)) {
      launch_gemm_small(p, S());
    } else {
      p.rowsum = nullptr;
      run_gemm(p);
      launch_sum_axis(dt, dz, g_b[l], 1, rows, n, 0, n, 1, S());
    }
    // the cotangent of the layer's input: dZ W (. hidden_act' of the layer below, whose output is a_in)
    if (l > 0 || gx) {
      Holder next;
      void* dst = l > 0 ? nullptr : scratch_or(gx, m, gxh);
      if (l > 0) {
        const int64_t d2[2] = {rows, m};
        next.t = new_tensor(2, d2, 0, dt);
        dst = next.t->ptr;
      }
      GemmProblem q = row_gemm(dt, dz, n, 1, w[l]->ptr, m, 1, dst, rows, m, n);
      if (l > 0) { q.dact = a_in; q.dact_kind = hk; }
      gemm_with_epilogue(q);
      if (l == 0) from_time_major(dst, gx, m);
      else { Holder drop(dz_cur.take()); dz_cur.t = next.take(); }
    }
  }
  if (sgd) {  // trainNetwork': s -= rate_state gs, every parameter -= rate_params g
    for (int l = 0; l < n_layers; ++l) {
      before_write(w[l]); before_write(b[l]);
      w[l]->id = fresh_id(); b[l]->id = fresh_id();
      launch_sgd(dt, w[l]->ptr, g_w[l], a.rate_params, w[l]->total(), S());
      launch_sgd(dt, b[l]->ptr, g_b[l], a.rate_params, b[l]->total(), S());
      if (state_act[l] != TO_RNN_STATELESS) {
        before_write(s[l]); before_write(ws[l]);
        s[l]->id = fresh_id(); ws[l]->id = fresh_id();
        launch_sgd(dt, s[l]->ptr, g_s[l], a.rate_state, s[l]->total(), S());
        launch_sgd(dt, ws[l]->ptr, g_ws[l], a.rate_params, ws[l]->total(), S());
      }
    }
  }
  TO_HIP(hipStreamSynchronize(S()));
}

to_status to_rnn_stack_run(int n_layers, const int* state_act, const to_tensor* s, const to_tensor* ws, const to_tensor* w,
                           const to_tensor* b, int hidden_act, int out_act, to_tensor X, to_tensor out,
                           const to_tensor* s_out_or_null) {
  API_BEGIN
  RnnStackArgs a{RnnMode::Run, n_layers, state_act, s, ws, w, b, hidden_act, out_act, X};
  a.out = out; a.s_out = s_out_or_null;
  rnn_stack_impl(a);
  API_END
}

to_status to_rnn_stack_grad(int n_layers, const int* state_act, const to_tensor* s, const to_tensor* ws, const to_tensor* w,
                            const to_tensor* b, int hidden_act, int out_act, int loss, to_tensor X, to_tensor Y,
                            const to_tensor* gs, const to_tensor* gws, const to_tensor* gw, const to_tensor* gb,
                            to_tensor gx_or_null, to_tensor losses_or_null) {
  API_BEGIN
  RnnStackArgs a{RnnMode::Grad, n_layers, state_act, s, ws, w, b, hidden_act, out_act, X, loss, Y};
  a.gs = gs; a.gws = gws; a.gw = gw; a.gb = gb; a.gx = gx_or_null; a.losses = losses_or_null;
  rnn_stack_impl(a);
  API_END
}

to_status to_rnn_stack_sgd(int n_layers, const int* state_act, const to_tensor* s, const to_tensor* ws, const to_tensor* w,
                           const to_tensor* b, int hidden_act, int out_act, int loss, to_tensor X, to_tensor Y,
                           double rate_state, double rate_params, to_tensor losses_or_null) {
  API_BEGIN
  RnnStackArgs a{RnnMode::Sgd, n_layers, state_act, s, ws, w, b, hidden_act, out_act, X, loss, Y};
  a.losses = losses_or_null; a.rate_state = rate_state; a.rate_params = rate_params;
  rnn_stack_impl(a);
  API_END
}

to_status to_set_rnn_persistent(int on, int* previous_or_null) {
  API_BEGIN
  TO_CHECK(on >= 0 && on <= 2, TO_ERR_ARG, "to_set_rnn_persistent: 0 (per step), 1 (automatic) or 2 (wherever in range)");
  if (previous_or_null) *previous_or_null = g_rnn_persistent;
  g_rnn_persistent = on;
  API_END
}

to_status to_rnn_stats(int64_t* persistent_runs, int64_t* stepwise_runs) {
  API_BEGIN
  if (persistent_runs) *persistent_runs = g_rnn_persistent_runs;
  if (stepwise_runs) *stepwise_runs = g_rnn_stepwise_runs;
  API_END
}

}  // extern "C"
