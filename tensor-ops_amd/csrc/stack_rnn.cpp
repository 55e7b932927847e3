// ---- recurrent stacks: `runNetwork` / `netGrad` / `trainNetwork'` of Recurrent.hs as one call -------------------------
// Layer l is `fullyConnected` (Recurrent.hs:91-119; z = W x + W' s + b, new state state_act[l](z) -- logistic or tanh, each
// layer its own --, output z through the layer's `*~ act`, hidden_act) or a stateless ffLayer (:126-138).  Internally everything is TIME-MAJOR, the rows of step t in one
// block (RnnRows: dense, row r = t * B + b; ragged, the packed rows of the sequences still running), so that every
// time-independent piece is ONE contraction over all N rows: the input projections (bias in the epilogue), the head,
// the weight gradients dZ^T X and dZ^T S_prev (+ the bias row sums) and the input cotangents dZ W (hidden_act' of the layer
// below in the epilogue).  Per stateful layer `prev` is the state before each step (block 0 = the initial states) and `after`
// the state after it.  What is left is each stateful layer's recurrence: persistent (rnn_seq.hip / rnn_ragged.hip, one launch
// per layer and direction for all steps) or per step (one GEMM with the addend, plus one elementwise launch).
// One validator (rnn_stack_check), one forward (rnn_forward), one backward (rnn_backward) and one update (rnn_apply_sgd) serve
// the dense entries, the ragged ones, generation's per-step route and online SGD's per-sequence route; dense and ragged
// differ in their RnnRows and in how rows move to and from the caller (rnn_rows_in / rnn_rows_out).
#include <algorithm>
#include <memory>

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
struct RnnStackArgs {  // what an entry has; each fills what it has
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
  const char* fn = nullptr;   // the entry's name in messages when it is none of the three dense ones
  const char* name() const {
    return fn ? fn : mode == RnnMode::Run ? "to_rnn_stack_run" : mode == RnnMode::Grad ? "to_rnn_stack_grad" : "to_rnn_stack_sgd";
  }
};
static int rnn_state_kind(int state_act) { return state_act == TO_ACT_TANH ? ACT_KIND_TANH : ACT_KIND_LOGISTIC; }

// ---- the time-major rows of a call ------------------------------------------------------------------------------------------
// Step t owns the cnt(t) rows from off(t) on.  Dense: all B sequences at every step, no table anywhere.  Ragged: the
// sequences sorted by length (rnn_ragged.hip), the first cnt(t) of them still running at step t.
struct RnnRows {
  int64_t B, T, N;                     // sequences; steps (ragged: of the longest); rows in all
  const RaggedTables* tb = nullptr;    // ragged: the schedule on the device
  const int* offs = nullptr;           // ragged: the same off[0 .. T] on the host
  int64_t off(int64_t t) const { return tb ? offs[t] : t * B; }
  int64_t cnt(int64_t t) const { return tb ? offs[t + 1] - offs[t] : B; }
};
static RnnRows dense_rows(int64_t B, int64_t T) { return {B, T, T * B}; }

static void* rnn_scratch(int dt, int64_t rows, int64_t n, Holder& h) {
  const int64_t d2[2] = {rows, n};
  h.t = new_tensor(2, d2, 0, dt);
  return h.t->ptr;
}

// ---- the forward over the rows of a call: the dense and the ragged entries (all steps of X) and to_rnn_stack_generate's
// per-step route (the prime, then each generated step with T = 1) ---------------------------------------------------------
struct RnnStateSrc {  // where a stateful layer's initial states are: one [n] for every sequence, or [B][n] (bstride apart)
  const void* ptr = nullptr;
  bool batched = false;
  int64_t bstride = 0, stride = 1;
};
static std::vector<RnnStateSrc> rnn_initial_states(int n_layers, const to_tensor* s) {
  std::vector<RnnStateSrc> init(n_layers);
  for (int l = 0; l < n_layers; ++l)
    if (s[l]) init[l] = {s[l]->ptr, s[l]->batch != 0, s[l]->bstride, s[l]->strides[0]};
  return init;
}
struct RnnForward {  // what the forward leaves behind
  std::vector<Holder> Z, Sa, Sp, WT, Ah;   // per layer: z [N][n]; the states (below); W'^T; hidden_act(z)
  // The state before each step (block 0: the initial states) and after it, row for row with Z.  Dense: two views of Sa
  // [(T+1)*B][n], B rows apart.  Ragged: Sp and Sa [N][n], for a step's rows are not the step before's.
  std::vector<void*> prev, after;
  std::vector<const void*> outp;       // what the layer above reads: hidden_act(z_l), all rows
  std::vector<RnnSeqPlan> plan;
  std::vector<char> persist;
  bool any_state = false, all_persistent = true;
  const void* no_bias_for_head = nullptr;  // stateless last layer of a run: the head launch adds b_L
  explicit RnnForward(int n)
      : Z(n), Sa(n), Sp(n), WT(n), Ah(n), prev(n, nullptr), after(n, nullptr), outp(n, nullptr), plan(n), persist(n, 0) {}
};

static void rnn_forward(int dt, int n_layers, const int* state_act, const RnnStateSrc* init, const to_tensor* ws,
                        const to_tensor* w, const to_tensor* b, int hk, bool run, const void* Xt, int64_t in_n,
                        const RnnRows& r, RnnForward& f) {
  const int64_t N = r.N, B = r.B, es = dt == TO_F64 ? 8 : 4;
  const void* below = Xt;
  int64_t below_n = in_n;
  for (int l = 0; l < n_layers; ++l) {
    const int64_t n = w[l]->dims[0];
    const bool last = l + 1 == n_layers, stateful = state_act[l] != TO_RNN_STATELESS;
    const int kind = rnn_state_kind(state_act[l]);
    void* z = rnn_scratch(dt, N, n, f.Z[l]);
    // the input projection (stateless hidden layer: its activation) over all rows
    GemmProblem p = row_gemm(dt, below, below_n, 1, w[l]->ptr, 1, below_n, z, N, n, below_n);
    p.bias = b[l]->ptr;
    if (!stateful && !last) p.act = hk + 1;
    if (last && !stateful && run) { p.bias = nullptr; f.no_bias_for_head = b[l]->ptr; }
    gemm_with_epilogue(p);
    if (stateful) {
      f.any_state = true;
      if (r.tb) {
        f.after[l] = rnn_scratch(dt, N, n, f.Sa[l]);
        f.prev[l] = rnn_scratch(dt, N, n, f.Sp[l]);
      } else {
        f.prev[l] = rnn_scratch(dt, N + B, n, f.Sa[l]);
        f.after[l] = at(f.prev[l], B * n, es);
      }
      void *sp = f.prev[l], *sa = f.after[l];
      if (!init[l].batched) {
        launch_bcast_axis(dt, init[l].ptr, sp, 1, B, n, 0, S());
      } else if (r.tb) {
        launch_ragged_states(dt, 0, *r.tb, init[l].ptr, sp, n, init[l].bstride, init[l].stride, S());
      } else {
        const int64_t dd[2] = {B, n}, ss[2] = {init[l].bstride, init[l].stride};
        launch_copy_strided(dt, init[l].ptr, sp, 2, dd, ss, S());
      }
      f.persist[l] = rnn_persistent_for(dt, n, B, &f.plan[l]);
      f.all_persistent = f.all_persistent && f.persist[l];
      if (f.persist[l]) {
        const int64_t dd[2] = {n, n}, ss[2] = {1, n};  // W'^T: M[k][j] = W'[j][k]
        f.WT[l].t = new_tensor(2, dd, 0, dt);
        launch_copy_strided(dt, ws[l]->ptr, f.WT[l].t->ptr, 2, dd, ss, S());
        if (r.tb) launch_rnn_ragged_seq(dt, false, f.plan[l], *r.tb, f.WT[l].t->ptr, z, sa, sp, n, kind, S());
        else launch_rnn_seq(dt, false, f.plan[l], f.WT[l].t->ptr, z, sp, B, r.T, n, kind, S());
      } else {
        // z_t = P_t + s_{t-1} W'^T (in place), s_t = state_act(z_t), on the step's rows; the states before step t >= 1 are
        // the first cnt(t) rows of `after`'s block t - 1
        for (int64_t t = 0; t < r.T; ++t) {
          const void* before = t == 0 ? sp : at(sa, r.off(t - 1) * n, es);
          GemmProblem q = row_gemm(dt, before, n, 1, ws[l]->ptr, 1, n, at(z, r.off(t) * n, es), r.cnt(t), n, n);
          q.beta = 1.0;
          q.Cin = q.C;
          gemm_with_epilogue(q);
          ew2(dt, kind == ACT_KIND_TANH ? EW_TANH : EW_LOGISTIC, at(sa, r.off(t) * n, es), at(z, r.off(t) * n, es), nullptr,
              r.cnt(t) * n);
        }
        if (r.tb && !run) launch_ragged_states(dt, 2, *r.tb, sa, sp, n, 0, 0, S());   // Sp blocks 1..: the left operand of gW'
      }
    }
    // what the layer above reads: a hidden stateful layer's output hidden_act(z) IS its state when the two activations
    // are the same function; otherwise it is one more elementwise pass over all rows of z
    if (stateful && !last && kind == hk) {
      below = f.after[l];
    } else if (stateful && !last) {
      void* ah = rnn_scratch(dt, N, n, f.Ah[l]);
      ew2(dt, hk == ACT_KIND_TANH ? EW_TANH : EW_LOGISTIC, ah, z, nullptr, N * n);
      below = ah;
    } else {
      below = z;
    }
    f.outp[l] = below;
    below_n = n;
  }
}

// out_act(z_L (+ b_L where the forward left it to the head)) of all `rows` rows into ot [rows][n_L]
// (zb holds the zero bias: the caller keeps it until the stream has run)
static void rnn_head_rows(int dt, const RnnForward& f, int n_layers, int64_t nL, int64_t rows, int out_act, void* ot,
                          Holder& zb) {
  const void* bias = f.no_bias_for_head;
  if (!bias) {
    if (!zb.t) {
      zb.t = new_tensor(1, &nL, 0, dt);
      launch_fill(dt, zb.t->ptr, nL, 0.0, S());
    }
    bias = zb.t->ptr;
  }
  launch_infer_rows(dt, f.Z[n_layers - 1].t->ptr, rows, bias, (int)nL, out_act == TO_ACT_SOFTMAX, ot, nullptr, 0, nullptr,
                    nullptr, S());
}

// ---- validation: nothing is produced, claimed or launched by any of this ------------------------------------------------
// at least one layer, every state activation, the hidden activation (returned as the kernels number it)
static int rnn_acts_check(const RnnStackArgs& a, const std::string& F) {
  TO_CHECK(a.n_layers >= 1, TO_ERR_ARG, F + "need at least one layer");
  for (int l = 0; l < a.n_layers; ++l)
    TO_CHECK(a.state_act[l] == TO_ACT_LOGISTIC || a.state_act[l] == TO_ACT_TANH || a.state_act[l] == TO_RNN_STATELESS,
             TO_ERR_UNSUPPORTED,
             F + "layer " + std::to_string(l) + ": the state activation must be logistic or tanh (or TO_RNN_STATELESS)");
  return stack_hidden_act_check(a.hidden_act);
}
// per layer: s and W' (none for a stateless layer) against W (checked before), their gradient destinations (grad) and the
// final-state destinations (run), all of X's dtype and batch
static void rnn_layers_check(const RnnStackArgs& a, const std::string& F) {
  const bool run = a.mode == RnnMode::Run, grad = a.mode == RnnMode::Grad;
  const to_tensor *s = a.s, *ws = a.ws, *s_out = a.s_out, *gs = a.gs, *gws = a.gws;
  const int dt = a.X->dtype;
  for (int l = 0; l < a.n_layers; ++l) {
    const int64_t n = a.w[l]->dims[0];
    const std::string L = F + "layer " + std::to_string(l) + ": ";
    if (a.state_act[l] == TO_RNN_STATELESS) {
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
      TO_CHECK(s[l]->batch == 0 || s[l]->batch == a.X->batch, TO_ERR_SHAPE,
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
      TO_CHECK(s_out[l]->rank == 1 && s_out[l]->dims[0] == n && s_out[l]->batch == a.X->batch && s_out[l]->contiguous(),
               TO_ERR_SHAPE, L + "s_out must be a contiguous [B; n] of X's batch, got " + shape_str(s_out[l]));
    }
  }
}

struct RnnChecked {  // what the validation derived
  int dt;
  int64_t T, B, nL;
  int hk, head;   // hidden_act as ACT_KIND_*; stack_loss_head's number (0 for run)
};
// Everything the dense entries require of their arguments; the ragged entries and online SGD (for one sequence of its X)
// require the same and add their own.
static RnnChecked rnn_stack_check(const RnnStackArgs& a) {
  const bool run = a.mode == RnnMode::Run, grad = a.mode == RnnMode::Grad;
  const int* state_act = a.state_act;   // (NONNULL reports its argument as spelt: the entries' parameter names)
  const to_tensor *s = a.s, *ws = a.ws, *w = a.w, *b = a.b, *gs = a.gs, *gws = a.gws, *gw = a.gw, *gb = a.gb;
  const to_tensor X = a.X, Y = a.Y, out = a.out, gx = a.gx, losses = a.losses;
  const std::string F = std::string(a.name()) + ": ";
  require_init();
  no_capture(a.name());
  NONNULL(state_act); NONNULL(s); NONNULL(ws); NONNULL(w); NONNULL(b); NONNULL(X);
  const int hk = rnn_acts_check(a, F);
  int head = 0;
  if (run)
    TO_CHECK(a.out_act == TO_ACT_SOFTMAX || a.out_act == TO_ACT_LOGISTIC, TO_ERR_UNSUPPORTED,
             F + "the output activation must be softmax or logistic");
  else
    head = stack_loss_head(a.out_act, a.loss, F);
  const int dt = X->dtype;
  TO_CHECK(X->rank == 2 && X->dims[0] >= 1 && X->dims[1] >= 1, TO_ERR_SHAPE,
           F + "X must be [B; T, i] (or [T, i]), got " + shape_str(X));
  const int64_t T = X->dims[0], B = X->batch > 0 ? X->batch : 1;
  if (grad) { NONNULL(gs); NONNULL(gws); NONNULL(gw); NONNULL(gb); }
  const int64_t nL = stack_params_check(a.n_layers, w, b, gw, gb, dt, X->dims[1]);
  auto seq_like = [&](to_tensor t, int64_t n, const char* what) {  // [B; T, n] of X's batch and dtype, contiguous
    TO_CHECK(t->dtype == dt, TO_ERR_ARG, F + what + " and X have different dtypes");
    TO_CHECK(t->rank == 2 && t->dims[0] == T && t->dims[1] == n && t->batch == X->batch, TO_ERR_SHAPE,
             F + what + " must be [B; " + std::to_string(T) + ", " + std::to_string(n) + "] of X's batch, got " + shape_str(t));
  };
  rnn_layers_check(a, F);
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
  return {dt, T, B, nL, hk, head};
}

// Operands produced, destinations claimed: the data `ins` and every parameter; the outputs `outs`, the final states and
// (grad) the gradient destinations.  Null entries are skipped.
static void rnn_ensure_claim(const RnnStackArgs& a, std::initializer_list<to_tensor> ins, std::initializer_list<to_tensor> outs) {
  for (to_tensor t : ins) if (t) ensure(t);
  for (int l = 0; l < a.n_layers; ++l) {
    ensure(a.w[l]); ensure(a.b[l]);
    if (a.s[l]) { ensure(a.s[l]); ensure(a.ws[l]); }
  }
  for (to_tensor t : outs) if (t) claim(t);
  if (a.s_out) for (int l = 0; l < a.n_layers; ++l) if (a.s_out[l]) claim(a.s_out[l]);
  if (a.mode == RnnMode::Grad)
    for (int l = 0; l < a.n_layers; ++l) {
      claim(a.gw[l]); claim(a.gb[l]);
      if (a.gs[l]) { claim(a.gs[l]); claim(a.gws[l]); }
    }
}

// the caller's [B; T, n] (any strides) as rows: t itself where it is time-major already (dense, B == 1), else one copy
static const void* rnn_rows_in(int dt, const RnnRows& r, to_tensor t, Holder& h) {
  if (!r.tb && r.B == 1 && t->contiguous()) return t->ptr;
  const int64_t n = t->dims[1], sb = t->batch > 0 ? t->bstride : 0;
  void* d = rnn_scratch(dt, r.N, n, h);
  if (r.tb) {
    launch_ragged_pack(dt, *r.tb, t->ptr, sb, t->strides[0], t->strides[1], d, n, S());
  } else {
    const int64_t d3[3] = {r.T, r.B, n}, s3[3] = {t->strides[0], sb, t->strides[1]};
    launch_copy_strided(dt, t->ptr, d, 3, d3, s3, S());
  }
  return d;
}
// where N x n values bound for dst (null: for nobody) are produced: scratch, or dst's own buffer where rnn_rows_out has
// nothing to move (dense, B == 1)
static void* rnn_rows_for(int dt, const RnnRows& r, to_tensor dst, int64_t n, Holder& h) {
  return dst && !r.tb && r.B == 1 ? dst->ptr : rnn_scratch(dt, r.N, n, h);
}
// rows [N][n] -> the caller's contiguous [B; T, n] (ragged: +0.0 at the padding)
static void rnn_rows_out(int dt, const RnnRows& r, const void* src, to_tensor dst, int64_t n) {
  if (src == dst->ptr) return;
  if (r.tb) return launch_ragged_unpack(dt, *r.tb, src, dst->ptr, dst->dims[0], n, S());
  const int64_t d3[3] = {r.B, r.T, n}, s3[3] = {n, r.B * n, 1};
  launch_copy_strided(dt, src, dst->ptr, 3, d3, s3, S());
}

// ---- the backward over the same rows ------------------------------------------------------------------------------------------
// gradient destinations: the caller's (grad) or scratch (sgd: applied at the end, so that a failure updates nothing)
struct RnnGrads {
  std::vector<Holder> scratch;
  std::vector<void*> s, ws, w, b;
  explicit RnnGrads(int n) : scratch(4 * n), s(n, nullptr), ws(n, nullptr), w(n), b(n) {}
};
static void rnn_grad_dests(const RnnStackArgs& a, int dt, RnnGrads& g) {
  for (int l = 0; l < a.n_layers; ++l) {
    auto dest = [&](const to_tensor* given, to_tensor like, Holder& h) -> void* {
      if (a.mode == RnnMode::Grad) return given[l]->ptr;
      h.t = new_tensor(like->rank, like->dims, 0, dt);
      return h.t->ptr;
    };
    g.w[l] = dest(a.gw, a.w[l], g.scratch[4 * l]);
    g.b[l] = dest(a.gb, a.b[l], g.scratch[4 * l + 1]);
    if (a.state_act[l] != TO_RNN_STATELESS) {
      g.s[l] = dest(a.gs, a.s[l], g.scratch[4 * l + 2]);
      g.ws[l] = dest(a.gws, a.ws[l], g.scratch[4 * l + 3]);
    }
  }
}

// dz_L = out_act(z_L) - y of every row (into dzL) and, if asked for, the per-row losses into the caller's [B; T]
static void rnn_loss_head(const RnnStackArgs& a, const RnnChecked& c, const RnnRows& r, const RnnForward& f, const void* Yt,
                          Holder& dzL) {
  const to_tensor losses = a.losses;
  Holder lh;
  void* dz = rnn_scratch(c.dt, r.N, c.nL, dzL);
  void* lt = losses ? rnn_rows_for(c.dt, r, losses, 1, lh) : nullptr;
  launch_loss_grad_rows(c.dt, f.Z[a.n_layers - 1].t->ptr, Yt, dz, lt, r.N, c.nL, loss_grad_rows_kind(c.head), S());
  if (!losses || lt == losses->ptr) return;
  if (r.tb) return rnn_rows_out(c.dt, r, lt, losses, 1);
  const int64_t dd[2] = {r.B, r.T}, ss[2] = {1, r.B};  // [T][B] -> [B][T]
  launch_copy_strided(c.dt, lt, losses->ptr, 2, dd, ss, S());
}

// From dz_L down: per layer the recurrence's share of dz, then gW', gs, gW, gb and the cotangent of the layer's input (gx at
// the bottom, if asked for).
static void rnn_backward(const RnnStackArgs& a, const RnnChecked& c, const RnnRows& r, const RnnForward& f, const void* Xt,
                         Holder& dzL, const RnnGrads& g) {
  const int dt = c.dt;
  const int64_t N = r.N, B = r.B, es = dt == TO_F64 ? 8 : 4;
  const to_tensor *ws = a.ws, *w = a.w;
  Holder dz_cur(dzL.take()), gxh;
  for (int l = a.n_layers - 1; l >= 0; --l) {
    const int64_t n = w[l]->dims[0], m = w[l]->dims[1];
    void* dz = dz_cur.t->ptr;
    if (a.state_act[l] != TO_RNN_STATELESS) {
      // dz_t = G_t + (dz_{t+1} W') (.) state_act'(s_t) where the sequence has a step t + 1, in place over G
      const int kind = rnn_state_kind(a.state_act[l]);
      void *sp = f.prev[l], *sa = f.after[l];
      if (f.persist[l] && r.tb) {
        launch_rnn_ragged_seq(dt, true, f.plan[l], *r.tb, ws[l]->ptr, dz, sa, sp, n, kind, S());
      } else if (f.persist[l]) {
        launch_rnn_seq(dt, true, f.plan[l], ws[l]->ptr, dz, sp, B, r.T, n, kind, S());
      } else {  // per step: D = (dz_{t+1} W') (.) state_act'(s_t), then dz_t += D on the cnt(t+1) rows that go on
        Holder dtmp;
        rnn_scratch(dt, B, n, dtmp);
        for (int64_t t = r.T - 2; t >= 0; --t) {
          GemmProblem q = row_gemm(dt, at(dz, r.off(t + 1) * n, es), n, 1, ws[l]->ptr, n, 1, dtmp.t->ptr, r.cnt(t + 1), n, n);
          q.dact = at(sa, r.off(t) * n, es);
          q.dact_kind = kind;
          gemm_with_epilogue(q);
          ew2(dt, EW_AFFINE, at(dz, r.off(t) * n, es), at(dz, r.off(t) * n, es), dtmp.t->ptr, r.cnt(t + 1) * n);
        }
      }
      // gW' = dZ^T S_prev ; gs = (sum_b dz_0[b]) W' (block 0 holds all B sequences)
      run_gemm(row_gemm(dt, dz, 1, n, sp, n, 1, g.ws[l], n, n, N));
      Holder dsum(new_tensor(1, &n, 0, dt));
      launch_sum_axis(dt, dz, dsum.t->ptr, 1, B, n, 0, n, 1, S());
      run_gemm(row_gemm(dt, dsum.t->ptr, n, 1, ws[l]->ptr, n, 1, g.s[l], 1, n, n));
    }
    // gW = dZ^T A_in (+ gb = the row sums of dZ)
    const void* a_in = l > 0 ? f.outp[l - 1] : Xt;
    GemmProblem p = row_gemm(dt, dz, 1, n, a_in, m, 1, g.w[l], n, m, N);
    p.rowsum = g.b[l];
    if (gemm_small_route(p)) {
      launch_gemm_small(p, S());
    } else {
      p.rowsum = nullptr;
      run_gemm(p);
      launch_sum_axis(dt, dz, g.b[l], 1, N, n, 0, n, 1, S());
    }
    // the cotangent of the layer's input: dZ W (. hidden_act' of the layer below, whose output is a_in)
    if (l > 0 || a.gx) {
      Holder next;
      void* dst = rnn_rows_for(dt, r, l > 0 ? nullptr : a.gx, m, l > 0 ? next : gxh);
      GemmProblem q = row_gemm(dt, dz, n, 1, w[l]->ptr, m, 1, dst, N, m, n);
      if (l > 0) { q.dact = a_in; q.dact_kind = c.hk; }
      gemm_with_epilogue(q);
      if (l == 0) rnn_rows_out(dt, r, dst, a.gx, m);
      else { Holder drop(dz_cur.take()); dz_cur.t = next.take(); }
    }
  }
}

// trainNetwork': s -= rate_state gs, every parameter -= rate_params g
static void rnn_apply_sgd(const RnnStackArgs& a, int dt, const RnnGrads& g) {
  const to_tensor *s = a.s, *ws = a.ws, *w = a.w, *b = a.b;
  for (int l = 0; l < a.n_layers; ++l) {
    before_write(w[l]); before_write(b[l]);
    w[l]->id = fresh_id(); b[l]->id = fresh_id();
    launch_sgd(dt, w[l]->ptr, g.w[l], a.rate_params, w[l]->total(), S());
    launch_sgd(dt, b[l]->ptr, g.b[l], a.rate_params, b[l]->total(), S());
    if (a.state_act[l] != TO_RNN_STATELESS) {
      before_write(s[l]); before_write(ws[l]);
      s[l]->id = fresh_id(); ws[l]->id = fresh_id();
      launch_sgd(dt, s[l]->ptr, g.s[l], a.rate_state, s[l]->total(), S());
      launch_sgd(dt, ws[l]->ptr, g.ws[l], a.rate_params, ws[l]->total(), S());
    }
  }
}

// ---- the driver: a checked call whose operands exist and whose destinations are claimed, over the rows r ---------------
// (persistent_runs / stepwise_runs: the entry family's counters)
static void rnn_stack_rows(const RnnStackArgs& a, const RnnChecked& c, const RnnRows& r, int64_t& persistent_runs,
                           int64_t& stepwise_runs) {
  const bool run = a.mode == RnnMode::Run;
  const int dt = c.dt, n_layers = a.n_layers;
  const int64_t es = dt == TO_F64 ? 8 : 4;
  Holder xh, yh;
  const void* Xt = rnn_rows_in(dt, r, a.X, xh);
  const void* Yt = !run ? rnn_rows_in(dt, r, a.Y, yh) : nullptr;
  RnnForward f(n_layers);
  rnn_forward(dt, n_layers, a.state_act, rnn_initial_states(n_layers, a.s).data(), a.ws, a.w, a.b, c.hk, run, Xt, a.X->dims[1],
              r, f);
  if (f.any_state) (f.all_persistent ? persistent_runs : stepwise_runs)++;
  if (run) {
    for (int l = 0; a.s_out && l < n_layers; ++l) {   // each sequence's state after its last step
      if (!a.s_out[l]) continue;
      const int64_t n = a.w[l]->dims[0];
      if (r.tb) launch_ragged_states(dt, 1, *r.tb, f.after[l], a.s_out[l]->ptr, n, 0, 0, S());
      else TO_HIP(hipMemcpyAsync(a.s_out[l]->ptr, at(f.after[l], r.off(r.T - 1) * n, es), (size_t)(r.B * n * es),
                                 hipMemcpyDeviceToDevice, S()));
    }
    Holder oh, zb;
    // (this late, behind the forward, is where the dense run has always checked it and its only check of it; a ragged call
    // has passed the same check before anything was enqueued, so for it this one cannot fire)
    TO_CHECK(c.nL <= 2147483647LL, TO_ERR_SHAPE, std::string(a.name()) + ": output layer too wide");
    void* ot = rnn_rows_for(dt, r, a.out, c.nL, oh);
    rnn_head_rows(dt, f, n_layers, c.nL, r.N, a.out_act, ot, zb);
    rnn_rows_out(dt, r, ot, a.out, c.nL);
    TO_HIP(hipStreamSynchronize(S()));
    return;
  }
  RnnGrads g(n_layers);
  rnn_grad_dests(a, dt, g);
  Holder dzL;
  rnn_loss_head(a, c, r, f, Yt, dzL);
  rnn_backward(a, c, r, f, Xt, dzL, g);
  if (a.mode == RnnMode::Sgd) rnn_apply_sgd(a, dt, g);   // after the whole backward: a failure before here updates nothing
  TO_HIP(hipStreamSynchronize(S()));
}

// the dense entries, and online SGD's per-sequence route on one sequence's views
static void rnn_stack_dense(const RnnStackArgs& a) {
  const RnnChecked c = rnn_stack_check(a);
  rnn_ensure_claim(a, {a.X, a.Y}, {a.out, a.gx, a.losses});
  rnn_stack_rows(a, c, dense_rows(c.B, c.T), g_rnn_persistent_runs, g_rnn_stepwise_runs);
}

to_status to_rnn_stack_run(int n_layers, const int* state_act, const to_tensor* s, const to_tensor* ws, const to_tensor* w,
                           const to_tensor* b, int hidden_act, int out_act, to_tensor X, to_tensor out,
                           const to_tensor* s_out_or_null) {
  API_BEGIN
  RnnStackArgs a{RnnMode::Run, n_layers, state_act, s, ws, w, b, hidden_act, out_act, X};
  a.out = out; a.s_out = s_out_or_null;
  rnn_stack_dense(a);
  API_END
}

to_status to_rnn_stack_grad(int n_layers, const int* state_act, const to_tensor* s, const to_tensor* ws, const to_tensor* w,
                            const to_tensor* b, int hidden_act, int out_act, int loss, to_tensor X, to_tensor Y,
                            const to_tensor* gs, const to_tensor* gws, const to_tensor* gw, const to_tensor* gb,
                            to_tensor gx_or_null, to_tensor losses_or_null) {
  API_BEGIN
  RnnStackArgs a{RnnMode::Grad, n_layers, state_act, s, ws, w, b, hidden_act, out_act, X, loss, Y};
  a.gs = gs; a.gws = gws; a.gw = gw; a.gb = gb; a.gx = gx_or_null; a.losses = losses_or_null;
  rnn_stack_dense(a);
  API_END
}

to_status to_rnn_stack_sgd(int n_layers, const int* state_act, const to_tensor* s, const to_tensor* ws, const to_tensor* w,
                           const to_tensor* b, int hidden_act, int out_act, int loss, to_tensor X, to_tensor Y,
                           double rate_state, double rate_params, to_tensor losses_or_null) {
  API_BEGIN
  RnnStackArgs a{RnnMode::Sgd, n_layers, state_act, s, ws, w, b, hidden_act, out_act, X, loss, Y};
  a.losses = losses_or_null; a.rate_state = rate_state; a.rate_params = rate_params;
  rnn_stack_dense(a);
  API_END
}

// ---- sequences of different lengths: to_rnn_stack_*_ragged ---------------------------------------------------------------
// Sequence b is steps 0 .. lens[b]-1 of X[b]; the rest of its rows is padding, never read.  The sequences are sorted by
// length (descending, stable) and their steps packed time-major (rnn_ragged.hip: at step t the first cnt[t] sorted positions
// are active and own the packed rows off[t] ..), N = sum lens rows in all.  That schedule is the call's RnnRows; everything
// else is the dense path's own code with rows = N.  Block 0 holds all B sequences, so gs is the dense expression too.  The
// recurrence: rnn_ragged_seq_kernel (one launch per layer and direction) or per step on the prefix of cnt[t] rows at off[t],
// by rnn_persistent_for -- the dense rule, measured on equal lengths only.  With every length equal to T the schedule IS the
// dense layout and every contraction the dense one.
static int64_t g_rnn_ragged_persistent_runs = 0, g_rnn_ragged_stepwise_runs = 0;

static void rnn_stack_ragged(const RnnStackArgs& a, const int64_t* lens) {
  const std::string F = std::string(a.fn) + ": ";
  const RnnChecked c = rnn_stack_check(a);   // the dense sibling's checks with its statuses
  NONNULL(lens);
  const int64_t T = c.T, B = c.B;
  int64_t Tmax = 0, N = 0;
  for (int64_t q = 0; q < B; ++q) {
    TO_CHECK(lens[q] >= 1 && lens[q] <= T, TO_ERR_SHAPE,
             F + "lens[" + std::to_string(q) + "] = " + std::to_string(lens[q]) + " is outside 1 .. T = " + std::to_string(T));
    Tmax = std::max(Tmax, lens[q]);
    N += lens[q];
  }
  TO_CHECK(c.nL <= 2147483647LL, TO_ERR_SHAPE, F + "output layer too wide");

  // ---- the row schedule: perm, its inverse, the lengths, off -- one table, one upload -------------------------------------
  std::vector<int> tab((size_t)(3 * B + Tmax + 1));
  int *perm = tab.data(), *inv = perm + B, *len32 = inv + B, *off = len32 + B;
  for (int64_t q = 0; q < B; ++q) { perm[q] = (int)q; len32[q] = (int)lens[q]; }
  std::stable_sort(perm, perm + B, [&](int x, int y) { return lens[x] > lens[y]; });
  for (int64_t p = 0; p < B; ++p) inv[perm[p]] = (int)p;
  std::vector<int64_t> cnt((size_t)Tmax + 1, 0);   // cnt[t]: sequences longer than t (cnt[Tmax] = 0)
  for (int64_t q = 0; q < B; ++q) cnt[lens[q] - 1]++;
  for (int64_t t = Tmax - 1; t >= 0; --t) cnt[t] += cnt[t + 1];
  off[0] = 0;
  for (int64_t t = 0; t < Tmax; ++t) off[t + 1] = off[t] + (int)cnt[t];

  rnn_ensure_claim(a, {a.X, a.Y}, {a.out, a.gx, a.losses});
  Holder tabh;
  const int64_t nw = (int64_t)tab.size();   // int32 in a float-typed pool buffer
  tabh.t = new_tensor(1, &nw, 0);
  host_to_device(tabh.t->ptr, tab.data(), tab.size() * sizeof(int), S());
  const int* dtab = static_cast<const int*>(tabh.t->ptr);
  const RaggedTables tb{dtab, dtab + B, dtab + 2 * B, dtab + 3 * B, (int)B, (int)Tmax, (int)N};
  rnn_stack_rows(a, c, RnnRows{B, Tmax, N, &tb, off}, g_rnn_ragged_persistent_runs, g_rnn_ragged_stepwise_runs);
}

to_status to_rnn_stack_run_ragged(int n_layers, const int* state_act, const to_tensor* s, const to_tensor* ws,
                                  const to_tensor* w, const to_tensor* b, int hidden_act, int out_act, to_tensor X,
                                  const int64_t* lens, to_tensor out, const to_tensor* s_out_or_null) {
  API_BEGIN
  RnnStackArgs a{RnnMode::Run, n_layers, state_act, s, ws, w, b, hidden_act, out_act, X};
  a.out = out; a.s_out = s_out_or_null; a.fn = "to_rnn_stack_run_ragged";
  rnn_stack_ragged(a, lens);
  API_END
}

to_status to_rnn_stack_grad_ragged(int n_layers, const int* state_act, const to_tensor* s, const to_tensor* ws,
                                   const to_tensor* w, const to_tensor* b, int hidden_act, int out_act, int loss, to_tensor X,
                                   to_tensor Y, const int64_t* lens, const to_tensor* gs, const to_tensor* gws,
                                   const to_tensor* gw, const to_tensor* gb, to_tensor gx_or_null, to_tensor losses_or_null) {
  API_BEGIN
  RnnStackArgs a{RnnMode::Grad, n_layers, state_act, s, ws, w, b, hidden_act, out_act, X, loss, Y};
  a.gs = gs; a.gws = gws; a.gw = gw; a.gb = gb; a.gx = gx_or_null; a.losses = losses_or_null;
  a.fn = "to_rnn_stack_grad_ragged";
  rnn_stack_ragged(a, lens);
  API_END
}

to_status to_rnn_stack_sgd_ragged(int n_layers, const int* state_act, const to_tensor* s, const to_tensor* ws,
                                  const to_tensor* w, const to_tensor* b, int hidden_act, int out_act, int loss, to_tensor X,
                                  to_tensor Y, const int64_t* lens, double rate_state, double rate_params,
                                  to_tensor losses_or_null) {
  API_BEGIN
  RnnStackArgs a{RnnMode::Sgd, n_layers, state_act, s, ws, w, b, hidden_act, out_act, X, loss, Y};
  a.losses = losses_or_null; a.rate_state = rate_state; a.rate_params = rate_params; a.fn = "to_rnn_stack_sgd_ragged";
  rnn_stack_ragged(a, lens);
  API_END
}

to_status to_rnn_ragged_stats(int64_t* persistent_runs, int64_t* stepwise_runs) {
  API_BEGIN
  if (persistent_runs) *persistent_runs = g_rnn_ragged_persistent_runs;
  if (stepwise_runs) *stepwise_runs = g_rnn_ragged_stepwise_runs;
  API_END
}

// ---- closed-loop generation: `runNetworkSt` under `iterate` as one call ---------------------------------------------------
// A generated step's input does not exist before the step before has finished, so the generated steps are a chain.  Per
// step (route A): the prime is the forward above on X, then per generated step one feed launch and that forward with T = 1
// on the carried states.  Persistent (route B, rnn_generate.hip): the prime and all G steps of all rows in ONE launch, the
// whole stack in LDS -- the prime too, so that a call's values do not depend on where a sequence is cut into calls.
static int g_rnn_generate_persistent = 1;   // to_set_rnn_generate_persistent: 0 per step, 1 auto, 2 wherever in range
static int64_t g_rnn_generate_persistent_runs = 0, g_rnn_generate_step_runs = 0;

// the widths (the input's first) and which layers have a state, as rnn_gen_plan / rnn_online_plan read them
struct RnnShape {
  int64_t widths[RNN_GEN_MAX_LAYERS + 1] = {};
  int stateful[RNN_GEN_MAX_LAYERS] = {};
  RnnShape(int n_layers, int64_t in_n, const int* state_act, const to_tensor* w) {   // n_layers <= RNN_GEN_MAX_LAYERS
    widths[0] = in_n;
    for (int l = 0; l < n_layers; ++l) {
      widths[l + 1] = w[l]->dims[0];
      stateful[l] = state_act[l] != TO_RNN_STATELESS;
    }
  }
};

to_status to_rnn_stack_generate(int n_layers, const int* state_act, const to_tensor* s, const to_tensor* ws, const to_tensor* w,
                                const to_tensor* b, int hidden_act, int out_act, int feed, to_tensor X, to_tensor U_or_null,
                                int64_t G, to_tensor prime_out_or_null, to_tensor out, int64_t* symbols_or_null,
                                const to_tensor* s_out_or_null) {
  API_BEGIN
  const char* fn = "to_rnn_stack_generate";
  const std::string F = std::string(fn) + ": ";
  const to_tensor U = U_or_null, prime_out = prime_out_or_null;
  const to_tensor* s_out = s_out_or_null;
  require_init();
  no_capture(fn);
  NONNULL(state_act); NONNULL(s); NONNULL(ws); NONNULL(w); NONNULL(b); NONNULL(X); NONNULL(out);
  RnnStackArgs a{RnnMode::Run, n_layers, state_act, s, ws, w, b, hidden_act, out_act, X};   // the stack as a run sees it
  a.s_out = s_out;
  const int hk = rnn_acts_check(a, F);
  TO_CHECK(out_act == TO_ACT_SOFTMAX || out_act == TO_ACT_LOGISTIC, TO_ERR_UNSUPPORTED,
           F + "the output activation must be softmax or logistic");
  TO_CHECK(feed == TO_FEED_OUTPUT || feed == TO_FEED_ARGMAX || feed == TO_FEED_SAMPLE, TO_ERR_ARG,
           F + "feed must be TO_FEED_OUTPUT, TO_FEED_ARGMAX or TO_FEED_SAMPLE");
  TO_CHECK(G >= 1, TO_ERR_ARG, F + "G must be at least 1");
  TO_CHECK((feed == TO_FEED_SAMPLE) == (U != nullptr), TO_ERR_ARG,
           F + "U is required for TO_FEED_SAMPLE and must be null otherwise");
  TO_CHECK(feed != TO_FEED_OUTPUT || !symbols_or_null, TO_ERR_ARG, F + "TO_FEED_OUTPUT feeds no symbol: symbols must be null");
  const int dt = X->dtype;
  TO_CHECK(X->rank == 2 && X->dims[0] >= 1 && X->dims[1] >= 1, TO_ERR_SHAPE,
           F + "X must be [B; Tp, i] (or [Tp, i]), got " + shape_str(X));
  const int64_t Tp = X->dims[0], B = X->batch > 0 ? X->batch : 1, in_n = X->dims[1];
  const int64_t nL = stack_params_check(n_layers, w, b, nullptr, nullptr, dt, in_n);
  TO_CHECK(nL == in_n, TO_ERR_SHAPE,
           F + "the output is fed back as the input: n_L = " + std::to_string(nL) + " but i = " + std::to_string(in_n));
  TO_CHECK(nL <= 2147483647LL, TO_ERR_SHAPE, F + "output layer too wide");
  rnn_layers_check(a, F);
  auto seq_like = [&](to_tensor t, int64_t len, const char* what) {  // a contiguous [B; len, n_L] of X's batch and dtype
    TO_CHECK(t->dtype == dt, TO_ERR_ARG, F + what + " and X have different dtypes");
    TO_CHECK(t->rank == 2 && t->dims[0] == len && t->dims[1] == nL && t->batch == X->batch, TO_ERR_SHAPE,
             F + what + " must be [B; " + std::to_string(len) + ", " + std::to_string(nL) + "] of X's batch, got " + shape_str(t));
    TO_CHECK(t->contiguous(), TO_ERR_ARG, F + what + " must be contiguous");
  };
  seq_like(out, G, "out");
  if (prime_out) seq_like(prime_out, Tp, "prime_out");
  if (U) {
    TO_CHECK(U->dtype == dt, TO_ERR_ARG, F + "U and X have different dtypes");
    TO_CHECK(U->rank == 1 && U->dims[0] == G && U->batch == X->batch, TO_ERR_SHAPE,
             F + "U must be [B; " + std::to_string(G) + "] of X's batch, got " + shape_str(U));
    TO_CHECK(U->contiguous(), TO_ERR_ARG, F + "U must be contiguous");
  }
  TO_CHECK(Tp * B <= 2147483647LL && G * B <= 2147483647LL, TO_ERR_SHAPE, F + "more than 2^31-1 rows");
  {  // an output may overlap neither an input, nor a parameter, nor another output
    std::vector<to_tensor> outs{out, prime_out}, ins{X, U};
    for (int l = 0; l < n_layers; ++l) {
      if (s_out) outs.push_back(s_out[l]);
      ins.push_back(s[l]); ins.push_back(ws[l]); ins.push_back(w[l]); ins.push_back(b[l]);
    }
    for (size_t o = 0; o < outs.size(); ++o) {
      bool bad = false;
      for (to_tensor in : ins) bad = bad || stack_overlap(outs[o], in);
      for (size_t q = 0; q < o; ++q) bad = bad || stack_overlap(outs[o], outs[q]);
      TO_CHECK(!bad, TO_ERR_ARG, F + "an output overlaps an input, a parameter or another output");
    }
  }
  // The route.  The automatic rule is set from tools/rnn_generate_scan.py's table (profiles/rnn_generate_scan.txt, DESIGN.md
  // section 3.3): the persistent kernel is ahead of route A -- 1.6x to 5x -- wherever the batch fits 256 workgroups with at
  // most four (row, column) items of the widest layer a thread (fp32 64 -> 128 -> 64: up to B = 2048), and 1.5x behind it at
  // eight items a thread (B = 4096): plain FMAs from LDS then lose to the per-step route's GEMMs.  Five to seven items: not
  // measured, route A.
  RnnGenPlan gplan;
  bool persistent = false;
  if (g_rnn_generate_persistent != 0 && n_layers <= RNN_GEN_MAX_LAYERS) {
    const RnnShape sh(n_layers, in_n, state_act, w);
    persistent = rnn_gen_plan(dt, n_layers, sh.widths, sh.stateful, B, &gplan) && (g_rnn_generate_persistent == 2 || gplan.few_items);
  }
  rnn_ensure_claim(a, {X, U}, {out, prime_out});

  const int64_t es = dt == TO_F64 ? 8 : 4;
  Holder symh;
  long long* sym = nullptr;
  if (feed != TO_FEED_OUTPUT) {
    const int64_t nl = (B * G * 8 + 3) / 4;  // B * G int64 in a float-typed pool buffer
    symh.t = new_tensor(1, &nl, 0);
    sym = reinterpret_cast<long long*>(symh.t->ptr);
  }
  Holder xh, ph, zb, xg, og;
  std::unique_ptr<RnnForward> cur;
  if (persistent) {
    // ---- route B: the prime and every generated step in one launch; the states, X and the outputs where the caller has them --
    RnnGenOperands o;
    o.L = n_layers;
    o.widths[0] = in_n;
    for (int l = 0; l < n_layers; ++l) {
      o.widths[l + 1] = w[l]->dims[0];
      o.state_kind[l] = !s[l] ? -1 : state_act[l] == TO_ACT_TANH ? ACT_KIND_TANH : ACT_KIND_LOGISTIC;
      o.W[l] = w[l]->ptr; o.b[l] = b[l]->ptr;
      if (s[l]) {
        o.WS[l] = ws[l]->ptr;
        o.s_in[l] = s[l]->ptr;
        o.s_sb[l] = s[l]->batch > 0 ? s[l]->bstride : 0;
        o.s_ss[l] = s[l]->strides[0];
        o.s_out[l] = s_out && s_out[l] ? s_out[l]->ptr : nullptr;
      }
    }
    o.X = X->ptr; o.x_sb = X->batch > 0 ? X->bstride : 0; o.x_st = X->strides[0]; o.x_sj = X->strides[1];
    o.prime_out = prime_out ? prime_out->ptr : nullptr;
    o.U = U ? U->ptr : nullptr; o.out = out->ptr; o.sym = sym;
    o.B = B; o.Tp = Tp; o.G = G; o.hidden_kind = hk; o.feed = feed; o.softmax = out_act == TO_ACT_SOFTMAX;
    launch_rnn_gen(dt, gplan, o, S());
    g_rnn_generate_persistent_runs++;
  } else {
    // ---- route A.  The prime: X [B; Tp, i] time-major, the forward, the head -------------------------------------------
    const RnnRows prime = dense_rows(B, Tp), gen = dense_rows(B, G), one = dense_rows(B, 1);
    const void* Xt = rnn_rows_in(dt, prime, X, xh);
    std::vector<RnnStateSrc> init = rnn_initial_states(n_layers, s);
    cur.reset(new RnnForward(n_layers));
    rnn_forward(dt, n_layers, state_act, init.data(), ws, w, b, hk, true, Xt, in_n, prime, *cur);
    void* pt = rnn_rows_for(dt, prime, prime_out, nL, ph);
    rnn_head_rows(dt, *cur, n_layers, nL, Tp * B, out_act, pt, zb);
    if (prime_out) rnn_rows_out(dt, prime, pt, prime_out, nL);
    const void* prev = at(pt, (Tp - 1) * B * nL, es);   // the last prime step's rows [B][n_L]
    for (int l = 0; l < n_layers; ++l)   // the carried states: those after the prime's last step, [B][n_l]
      if (s[l]) init[l] = {at(cur->after[l], (Tp - 1) * B * w[l]->dims[0], es), true, w[l]->dims[0], 1};
    // per generated step one feed launch, then the forward with T = 1 on the carried states
    void* x = rnn_scratch(dt, B, in_n, xg);
    void* ot = rnn_rows_for(dt, gen, out, nL, og);   // time-major [G][B][n_L]
    for (int64_t k = 0; k < G; ++k) {
      launch_rnn_feed(dt, prev, B, nL, feed, U ? U->ptr : nullptr, G, k, x, sym, S());
      std::unique_ptr<RnnForward> nxt(new RnnForward(n_layers));
      rnn_forward(dt, n_layers, state_act, init.data(), ws, w, b, hk, true, x, in_n, one, *nxt);
      void* row = at(ot, k * B * nL, es);
      rnn_head_rows(dt, *nxt, n_layers, nL, B, out_act, row, zb);
      prev = row;
      for (int l = 0; l < n_layers; ++l)
        if (s[l]) init[l].ptr = nxt->after[l];
      cur = std::move(nxt);   // (the step before's buffers go back to the pool; the stream runs in order)
    }
    rnn_rows_out(dt, gen, ot, out, nL);
    if (s_out)
      for (int l = 0; l < n_layers; ++l)
        if (s_out[l])
          TO_HIP(hipMemcpyAsync(s_out[l]->ptr, init[l].ptr, (size_t)(B * w[l]->dims[0] * es), hipMemcpyDeviceToDevice, S()));
    g_rnn_generate_step_runs++;
  }
  if (symbols_or_null) device_to_host(symbols_or_null, sym, (size_t)(B * G) * sizeof(int64_t), S());
  TO_HIP(hipStreamSynchronize(S()));
  API_END
}

to_status to_set_rnn_generate_persistent(int on, int* previous_or_null) {
  API_BEGIN
  TO_CHECK(on >= 0 && on <= 2, TO_ERR_ARG,
           "to_set_rnn_generate_persistent: 0 (per step), 1 (automatic) or 2 (wherever in range)");
  if (previous_or_null) *previous_or_null = g_rnn_generate_persistent;
  g_rnn_generate_persistent = on;
  API_END
}

to_status to_rnn_generate_stats(int64_t* persistent_runs, int64_t* per_step_runs) {
  API_BEGIN
  if (persistent_runs) *persistent_runs = g_rnn_generate_persistent_runs;
  if (per_step_runs) *per_step_runs = g_rnn_generate_step_runs;
  API_END
}

// ---- per-sequence training: `trainNetwork'` folded over a set of sequences as one call --------------------------------------
// Step j trains on sequence idx[j] alone, from the parameters and learned initial states step j - 1 left: a dependent chain
// of single sequences.  Per sequence (route A): rnn_stack_dense in Sgd mode on the B = 1 views to_batch_select would give --
// bit for bit the caller's own loop of to_rnn_stack_sgd.  Persistent (route B, rnn_online.hip): all n_idx sequences in ONE
// launch by one workgroup, the whole stack in LDS.
static int g_rnn_online_persistent = 1;   // to_set_rnn_online_persistent: 0 per sequence, 1 auto, 2 wherever in range
static int64_t g_rnn_online_persistent_runs = 0, g_rnn_online_sequence_runs = 0;
// The automatic rule: route B where its plan fits AND no layer (the input not counted) is wider than H*.  H* = 128 is the
// largest width tools/rnn_online_scan.py scanned, and route B was ahead of route A at every scanned width at both T
// (profiles/rnn_online_scan.txt, fp32 64 -> H (stateful) -> 10: A / B = 4.8 / 1.7 at H = 32, 3.6 / 1.5 at 64, 3.2 / 1.4 at 96,
// 2.9 / 1.2 at 128, for T = 8 / 64).  Wider layers that still fit the LDS (up to about 200 columns in
// fp32) have not been measured and take route A.
constexpr int64_t RNN_ONLINE_AUTO_MAX_WIDTH = 128;
// Sequences of their own lengths (to_rnn_stack_online_sgd_ragged): step j trains on the leading lens[idx[j]] steps of its
// sequence; the rows behind them are padding, never read.  Route A: the same per-sequence calls on the views of the leading
// rows -- contiguous, for a sequence's leading rows are -- with losses zeroed once up front.  Route B: the same kernel with
// the step loops bounded by a device table of the n_idx lengths, its plan made for the longest length the call uses.  The
// route is chosen as for the dense entry; that rule was measured on equal lengths and, by tools/rnn_online_ragged_scan.py,
// on lengths uniform in 1 .. 64 (profiles/rnn_online_ragged_scan.txt).
static int64_t g_rnn_online_ragged_persistent_runs = 0, g_rnn_online_ragged_sequence_runs = 0;

// the dense entry (ragged false: lens is not looked at) and the ragged one
static void rnn_online_sgd(const char* fn, int n_layers, const int* state_act, const to_tensor* s, const to_tensor* ws,
                           const to_tensor* w, const to_tensor* b, int hidden_act, int out_act, int loss, to_tensor X, to_tensor Y,
                           bool ragged, const int64_t* lens, int64_t n_idx, const int64_t* idx, double rate_state,
                           double rate_params, to_tensor losses, int64_t& persistent_runs, int64_t& sequence_runs) {
  const std::string F = std::string(fn) + ": ";
  require_init();
  no_capture(fn);
  NONNULL(state_act); NONNULL(s); NONNULL(ws); NONNULL(w); NONNULL(b); NONNULL(X); NONNULL(Y);
  TO_CHECK(n_idx >= 1, TO_ERR_ARG, F + "n_idx must be at least 1");
  auto set_like = [&](to_tensor t, const char* what) {
    TO_CHECK(t->rank == 2 && t->batch > 0 && t->contiguous(), TO_ERR_SHAPE,
             F + what + " must be a batched, contiguous [N; T, n], got " + shape_str(t));
  };
  set_like(X, "X");
  set_like(Y, "Y");
  const int64_t N = X->batch, T = X->dims[0];
  const int dt = X->dtype;
  TO_CHECK(Y->batch == N, TO_ERR_SHAPE, F + "X and Y have different batches");
  // the stack, the pair and one sequence's shapes: to_rnn_stack_sgd's checks on what to_batch_select would hand it
  to_tensor_s xv, yv, lv;
  auto one_of = [](to_tensor_s& v, to_tensor t) {
    v.dtype = t->dtype;
    v.rank = t->rank;
    for (int d = 0; d < t->rank; ++d) { v.dims[d] = t->dims[d]; v.strides[d] = t->strides[d]; }
  };
  one_of(xv, X);
  one_of(yv, Y);
  RnnStackArgs chk{RnnMode::Sgd, n_layers, state_act, s, ws, w, b, hidden_act, out_act, &xv, loss, &yv};
  chk.fn = fn;
  if (losses) {
    TO_CHECK(losses->dtype == dt, TO_ERR_ARG, F + "losses and X have different dtypes");
    TO_CHECK(losses->rank == 1 && losses->dims[0] == T && losses->batch == n_idx && losses->contiguous(), TO_ERR_SHAPE,
             F + "losses must be a contiguous [" + std::to_string(n_idx) + "; " + std::to_string(T) + "], got " + shape_str(losses));
    one_of(lv, losses);
    chk.losses = &lv;
  }
  rnn_stack_check(chk);
  TO_CHECK(idx || n_idx <= N, TO_ERR_SHAPE, F + "more sequences asked for than X holds");
  for (int64_t j = 0; idx && j < n_idx; ++j)
    TO_CHECK(idx[j] >= 0 && idx[j] < N, TO_ERR_SHAPE, F + "sequence index out of range");
  if (losses) {
    bool bad = stack_overlap(losses, X) || stack_overlap(losses, Y);
    for (int l = 0; l < n_layers; ++l)
      bad = bad || stack_overlap(losses, s[l]) || stack_overlap(losses, ws[l]) || stack_overlap(losses, w[l]) || stack_overlap(losses, b[l]);
    TO_CHECK(!bad, TO_ERR_ARG, F + "losses overlaps X, Y or a parameter");
  }
  int64_t Tused = T;   // the longest sequence the call trains on
  std::vector<int64_t> steps;   // ragged: lens gathered by idx, as the kernel reads them
  if (ragged) {
    NONNULL(lens);
    for (int64_t q = 0; q < N; ++q)
      TO_CHECK(lens[q] >= 1 && lens[q] <= T, TO_ERR_SHAPE,
               F + "lens[" + std::to_string(q) + "] = " + std::to_string(lens[q]) + " is outside 1 .. T = " + std::to_string(T));
    steps.resize((size_t)n_idx);
    for (int64_t j = 0; j < n_idx; ++j) steps[j] = lens[idx ? idx[j] : j];
    Tused = *std::max_element(steps.begin(), steps.end());
  }
  // The route (RNN_ONLINE_AUTO_MAX_WIDTH above).
  RnnOnlinePlan plan;
  bool persistent = false;
  if (g_rnn_online_persistent != 0 && n_layers <= RNN_GEN_MAX_LAYERS) {
    const RnnShape sh(n_layers, X->dims[1], state_act, w);
    persistent = rnn_online_plan(dt, n_layers, sh.widths, sh.stateful, Tused, &plan) &&
                 (g_rnn_online_persistent == 2 || plan.nmax <= RNN_ONLINE_AUTO_MAX_WIDTH);
  }

  rnn_ensure_claim(chk, {X, Y}, {losses});
  if (persistent) {
    RnnOnlineOperands o;
    o.L = n_layers;
    o.widths[0] = X->dims[1];
    for (int l = 0; l < n_layers; ++l) {   // in-place writes: recorded readers of the old values first, new identities after
      claim(w[l]); claim(b[l]);
      o.widths[l + 1] = w[l]->dims[0];
      o.state_kind[l] = !s[l] ? -1 : state_act[l] == TO_ACT_TANH ? ACT_KIND_TANH : ACT_KIND_LOGISTIC;
      o.W[l] = w[l]->ptr; o.b[l] = b[l]->ptr;
      if (s[l]) {
        claim(s[l]); claim(ws[l]);
        o.WS[l] = ws[l]->ptr; o.s[l] = s[l]->ptr;
      }
    }
    Holder order, count, tape;
    auto upload = [&](const int64_t* host, Holder& h) {
      const int64_t nl = (n_idx * 8 + 3) / 4;   // n_idx int64 in a float-typed pool buffer
      h.t = new_tensor(1, &nl, 0);
      host_to_device(h.t->ptr, host, (size_t)n_idx * sizeof(int64_t), S());
      return static_cast<const long long*>(h.t->ptr);
    };
    if (idx) o.idx = upload(idx, order);
    if (ragged) o.lens = upload(steps.data(), count);
    if (!plan.tape_lds) {
      tape.t = new_tensor(1, &plan.tape_elems, 0, dt);
      o.tape = tape.t->ptr;
    }
    o.X = X->ptr; o.Y = Y->ptr; o.losses = losses ? losses->ptr : nullptr;
    o.n_idx = n_idx; o.T = T;
    o.hidden_kind = hidden_act == TO_ACT_TANH ? ACT_KIND_TANH : ACT_KIND_LOGISTIC;
    o.softmax = out_act == TO_ACT_SOFTMAX;
    o.rate_state = rate_state; o.rate_params = rate_params;
    launch_rnn_online(dt, plan, o, S());
    TO_HIP(hipStreamSynchronize(S()));   // the order, the lengths and the tape go back to the pool
    persistent_runs++;
  } else {
    if (ragged && losses) launch_fill(dt, losses->ptr, n_idx * T, 0.0, S());   // +0.0 at the padding
    for (int64_t j = 0; j < n_idx; ++j) {
      const int64_t q = idx ? idx[j] : j, len = ragged ? lens[q] : T;   // the leading len rows: all T of the dense entry
      const int64_t xd[2] = {len, X->dims[1]}, yd[2] = {len, Y->dims[1]};
      Holder xq(new_view(X, 2, xd, X->strides, 0, xd[0] * xd[1], q * X->bstride));
      Holder yq(new_view(Y, 2, yd, Y->strides, 0, yd[0] * yd[1], q * Y->bstride));
      Holder lq(losses ? new_view(losses, 1, &len, losses->strides, 0, len, j * losses->numel()) : nullptr);
      RnnStackArgs a{RnnMode::Sgd, n_layers, state_act, s, ws, w, b, hidden_act, out_act, xq.t, loss, yq.t};
      a.losses = lq.t; a.rate_state = rate_state; a.rate_params = rate_params; a.fn = fn;
      rnn_stack_dense(a);
    }
    sequence_runs++;
  }
}

to_status to_rnn_stack_online_sgd(int n_layers, const int* state_act, const to_tensor* s, const to_tensor* ws, const to_tensor* w,
                                  const to_tensor* b, int hidden_act, int out_act, int loss, to_tensor X, to_tensor Y,
                                  int64_t n_idx, const int64_t* idx_or_null, double rate_state, double rate_params,
                                  to_tensor losses_or_null) {
  API_BEGIN
  rnn_online_sgd("to_rnn_stack_online_sgd", n_layers, state_act, s, ws, w, b, hidden_act, out_act, loss, X, Y, false, nullptr,
                 n_idx, idx_or_null, rate_state, rate_params, losses_or_null, g_rnn_online_persistent_runs,
                 g_rnn_online_sequence_runs);
  API_END
}

to_status to_rnn_stack_online_sgd_ragged(int n_layers, const int* state_act, const to_tensor* s, const to_tensor* ws,
                                         const to_tensor* w, const to_tensor* b, int hidden_act, int out_act, int loss,
                                         to_tensor X, to_tensor Y, const int64_t* lens, int64_t n_idx,
                                         const int64_t* idx_or_null, double rate_state, double rate_params,
                                         to_tensor losses_or_null) {
  API_BEGIN
  rnn_online_sgd("to_rnn_stack_online_sgd_ragged", n_layers, state_act, s, ws, w, b, hidden_act, out_act, loss, X, Y, true, lens,
                 n_idx, idx_or_null, rate_state, rate_params, losses_or_null, g_rnn_online_ragged_persistent_runs,
                 g_rnn_online_ragged_sequence_runs);
  API_END
}

to_status to_rnn_online_ragged_stats(int64_t* persistent_runs, int64_t* per_sequence_runs) {
  API_BEGIN
  if (persistent_runs) *persistent_runs = g_rnn_online_ragged_persistent_runs;
  if (per_sequence_runs) *per_sequence_runs = g_rnn_online_ragged_sequence_runs;
  API_END
}

to_status to_set_rnn_online_persistent(int on, int* previous_or_null) {
  API_BEGIN
  TO_CHECK(on >= 0 && on <= 2, TO_ERR_ARG,
           "to_set_rnn_online_persistent: 0 (per sequence), 1 (automatic) or 2 (wherever in range)");
  if (previous_or_null) *previous_or_null = g_rnn_online_persistent;
  g_rnn_online_persistent = on;
  API_END
}

to_status to_rnn_online_stats(int64_t* persistent_runs, int64_t* per_sequence_runs) {
  API_BEGIN
  if (persistent_runs) *persistent_runs = g_rnn_online_persistent_runs;
  if (per_sequence_runs) *per_sequence_runs = g_rnn_online_sequence_runs;
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
