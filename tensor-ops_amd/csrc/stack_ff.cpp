// The one-call entry points for ffLayer stacks: to_fflayer_stack_grad / _sgd / _minibatch_sgd / _online_sgd / _infer / _induce,
// and for encoder / decoder pairs of them: to_autoencoder_stack_run / _decode / _grad / _sgd / _minibatch_sgd.
#include <deque>

#include "api_util.hpp"
#include "stack_util.hpp"

using namespace to;

extern "C" {

// A contraction of the step (row_gemm) with its fused epilogue (bias, act, dact).  A loss head (loss_rows) and, behind it, a
// tail (tail_n) on p are wishes: what the kernel taking p cannot fuse is dropped.  Returns the problem as it will be
// launched: loss_rows still set means C holds dz instead of z, tail_n still set that the tail is produced.  Decided by the
// shape alone, and launches nothing: to_fflayer_stack_minibatch_sgd asks it for every problem of its steps beforehand.
static GemmProblem fused_route(GemmProblem p) {
  // latency-bound shapes (incl. the tiny ones of a one-sample step) run on the small-GEMM kernel: it carries
  // every fused epilogue for both element types (the tiled fp64 kernel has none)
  const bool small = gemm_small_takes(p);
  if (!small || !gemm_small_fuses_loss(p)) { p.loss_rows = 0; p.target = nullptr; p.loss_out = nullptr; }
  if (!p.loss_rows || !p.tail_n || !gemm_small_fuses_tail(p, p.tail_n)) {
    p.tail_w = p.tail_h = nullptr; p.tail_out = nullptr; p.tail_n = 0; p.tail_kind = 0;
  }
  // the tiled fp64 kernel has no fused epilogue: the caller (the trainer) falls back to the generic path
  TO_CHECK(small || p.dtype == TO_F32, TO_ERR_UNSUPPORTED, "pre-fused fp64 path: a contraction is outside the small-GEMM range");
  return p;
}

static GemmProblem fused_gemm(GemmProblem p) {
  p = fused_route(p);
  if (gemm_small_takes(p)) launch_gemm_small(p, S());
  else launch_gemm_mfma(p, S());
  return p;
}

// One step of a stack -- the gradients of to_fflayer_stack_grad, or (sgd) the `trainNetwork` update -- with everything about
// it that does not depend on the batch: what fflayer_stack_impl and to_fflayer_stack_minibatch_sgd share.
// sgd: gw/gb are the parameters themselves and the weight-gradient launches apply
// P <- P - rate * gradient in their epilogue (alpha = -rate, beta = 1, Cin = C = W; the bias through the
// accumulating row sum): the step loses its separate update launch.
// act[l], l < n_layers - 1: the activation behind layer l (ACT_KIND_*; ACT_KIND_IDENTITY: none -- act = 0 in the forward, no
// dact in the backward and no fused tail behind it).  head_kind: stack_loss_head's pairs 1 / 2, which the small-GEMM kernel
// fuses (loss_rows) and launch_loss_grad_rows knows, or the pairs 3 / 4 of ae_loss_head, which never set loss_rows: their
// head is launch_recon_head behind the last GEMM.
struct StackStep {
  int n_layers;
  const to_tensor *w, *b, *gw, *gb;
  const int* act;
  int head_kind, dt;
  bool sgd;
  double rate;

  // The weight gradient of layer l (dz_l^T . a_in, + its row sums = the bias gradient) as a GEMM problem:
  // A element (i,k) = dz[k*n + i], B element (k,j) = a_in[k*m + j]
  GemmProblem wgrad(int l, const void* dz, const void* a_in, int64_t B) const {
    const int64_t n = w[l]->dims[0], m = w[l]->dims[1];
    GemmProblem p = row_gemm(dt, dz, 1, n, a_in, m, 1, gw[l]->ptr, n, m, B);
    p.rowsum = gb[l]->ptr;
    if (sgd) {
      p.alpha = -rate; p.beta = 1.0; p.Cin = w[l]->ptr;
      p.rowsum_acc = true; p.rowsum_alpha = -rate;
    }
    return p;
  }
  // forward, layer l: C[B,n] = A[B,prev_n] . W^T : B operand element (k, j) = W[j*prev_n + k]; bias and the hidden
  // activation in the epilogue; the last layer wishes for the loss head and (two layers or more) for the tail
  // dz_{L-1} = (dz_L . W_L) * act'(h) of its rows in the same launch
  GemmProblem forward(int l, const void* prev, void* C, int64_t B, const void* y, void* losses, const void* h,
                      void* tail_out) const {
    static const int fuse_tail = [] { const char* e = ab_getenv("TOPS_STEP_FUSE_TAIL"); return e ? atoi(e) : 1; }();
    const int64_t n = w[l]->dims[0], prev_n = w[l]->dims[1];
    const bool last = l + 1 == n_layers;
    GemmProblem p = row_gemm(dt, prev, prev_n, 1, w[l]->ptr, 1, prev_n, C, B, n, prev_n);
    p.bias = b[l]->ptr;
    p.act = last ? 0 : act[l] + 1;
    if (last && head_kind <= 2) { p.loss_rows = head_kind; p.target = y; p.loss_out = losses; }
    if (last && head_kind <= 2 && n_layers >= 2 && fuse_tail && act[l - 1] != ACT_KIND_IDENTITY) {
      p.tail_w = w[l]->ptr; p.tail_h = h; p.tail_out = tail_out; p.tail_n = (int)prev_n; p.tail_kind = act[l - 1];
    }
    return p;
  }
  bool wants_tail() const { return forward(n_layers - 1, nullptr, nullptr, 1, nullptr, nullptr, nullptr, nullptr).tail_n != 0; }
  // dz_{l-1}[B,m] = (dz_l[B,n] . W_l[n,m]) * act'(h), h = act[l-1]  (h (1 - h), or 1 - h h for tanh)
  GemmProblem backward(int l, const void* dz, const void* h, void* out, int64_t B) const {
    const int64_t n = w[l]->dims[0], m = w[l]->dims[1];
    GemmProblem q = row_gemm(dt, dz, n, 1, w[l]->ptr, m, 1, out, B, m, n);
    if (act[l - 1] != ACT_KIND_IDENTITY) { q.dact = h; q.dact_kind = act[l - 1]; }
    return q;
  }

  // nothing may be half-updated: every weight gradient of an sgd step must be one small-GEMM launch
  void check_wgrads(int64_t B) const {
    if (!sgd) return;
    for (int l = 0; l < n_layers; ++l)
      TO_CHECK(gemm_small_takes(wgrad(l, nullptr, nullptr, B)), TO_ERR_UNSUPPORTED,
               "fused SGD step: a weight gradient is outside the small-GEMM range");
  }
  // Every refusal the launches of an sgd step on B rows can end in, with nothing launched: the same problems in the same
  // order, their routes decided by fused_route as launch() decides them.
  void check_sgd(int64_t B) const {
    check_wgrads(B);
    GemmProblem fwd{};
    for (int l = 0; l < n_layers; ++l) fwd = fused_route(forward(l, nullptr, nullptr, B, nullptr, nullptr, nullptr, nullptr));
    for (int l = n_layers - 1; l > 0; --l)
      if (!(l == n_layers - 1 && fwd.tail_n)) fused_route(backward(l, nullptr, nullptr, nullptr, B));
  }
  // ... and of a step of either kind: the weight gradients' walk as well, dry
  void check_step(int64_t B) const {
    check_sgd(B);
    wgrads(nullptr, nullptr, B, true);
  }
  void wgrads(const void* const* dz, const void* const* a_in, int64_t B, bool dry) const;
  void launch(const void* x, const void* y, void* losses, int64_t B) const;
};

// The launches of one step on the contiguous rows x [B; i0], y [B; n_L] (losses: B scalars, or null).  Operands exist and
// destinations are claimed.
void StackStep::launch(const void* x, const void* y, void* losses, int64_t B) const {
  Holder tail;  // dz_{L-1} when the last layer's launch produced it
  GemmProblem fwd{};  // the last layer's launch
  // forward: a_l = act(a_{l-1} W_l^T + b_l) for hidden layers (act: hidden_act), z_L for the last
  std::vector<Holder> a(n_layers);  // a[l]: [B; n_l]; the last holds z_L, then is reused as dz_L
  const void* prev = x;
  for (int l = 0; l < n_layers; ++l) {
    const int64_t n = w[l]->dims[0], prev_n = w[l]->dims[1];
    a[l].t = new_tensor(1, &n, B, dt);
    // (last layer: the loss head runs in the same launch when the row fits one 16-wide tile; it also produces
    //  dz_{L-1} for its rows where the tail fuses)
    const bool last = l + 1 == n_layers;
    if (last && wants_tail()) tail.t = new_tensor(1, &prev_n, B, dt);
    fwd = fused_gemm(forward(l, prev, a[l].t->ptr, B, y, losses, l > 0 ? a[l - 1].t->ptr : nullptr,
                             tail.t ? tail.t->ptr : nullptr));
    prev = a[l].t->ptr;
  }
  // loss gradient wrt z_L, per sample row
  const int64_t nL = w[n_layers - 1]->dims[0];
  Holder cur;
  if (fwd.loss_rows) {
    cur.t = a[n_layers - 1].t;  // already dz_L
    a[n_layers - 1].t = nullptr;
  } else if (head_kind <= 2) {
    cur.t = new_tensor(1, &nL, B, dt);
    launch_loss_grad_rows(dt, a[n_layers - 1].t->ptr, y, cur.t->ptr, losses, B, nL, loss_grad_rows_kind(head_kind), S());
  } else {  // z_L -> dz_L in place (the bias went in with the GEMM's epilogue)
    cur.t = a[n_layers - 1].t;
    a[n_layers - 1].t = nullptr;
    launch_recon_head(dt, head_kind, cur.t->ptr, nullptr, y, nL, cur.t->ptr, nullptr, losses, B, nL, S());
  }
  auto a_in = [&](int l) -> const void* { return l > 0 ? a[l - 1].t->ptr : x; };
  // backward, phase 1: every dz_l (the propagation reads W_l, which phase 2 may overwrite in place)
  std::vector<Holder> dz(n_layers);
  dz[n_layers - 1].t = cur.take();
  for (int l = n_layers - 1; l > 0; --l) {
    if (l == n_layers - 1 && fwd.tail_out) {
      dz[l - 1].t = tail.take();  // came out of the loss-head launch
    } else {
      const int64_t m = w[l]->dims[1];
      dz[l - 1].t = new_tensor(1, &m, B, dt);
      fused_gemm(backward(l, dz[l].t->ptr, a[l - 1].t->ptr, dz[l - 1].t->ptr, B));
    }
  }
  // phase 2: the weight gradients
  std::vector<const void*> dzp((size_t)n_layers), ap((size_t)n_layers);
  for (int l = 0; l < n_layers; ++l) { dzp[(size_t)l] = dz[l].t->ptr; ap[(size_t)l] = a_in(l); }
  wgrads(dzp.data(), ap.data(), B, false);
}

// The weight gradients of a step, independent of each other: dz[l] / a_in[l] per layer.  dry: the same walk with its
// refusals and nothing launched (dz / a_in null) -- check_step asks it, so what is refused is decided in ONE place.
// The two last ones go out as ONE launch when
// their shapes allow (one launch floor, ~4 us, less per step: 33.6 -> 28.0 us on config 3).
// (Running them on a side stream instead measured slower: the fork/join events cost more than the overlap
// buys, 0.0485 -> 0.0591 ms/step.)
void StackStep::wgrads(const void* const* dz, const void* const* a_in, int64_t B, bool dry) const {
  auto grad = [&](int l) { return wgrad(l, dry ? nullptr : dz[l], dry ? nullptr : a_in[l], B); };
  // one sample: every weight gradient is an outer product -- all layers in one launch
  static const int rank1 = [] { const char* e = ab_getenv("TOPS_STEP_RANK1"); return e ? atoi(e) : 1; }();
  if (B == 1 && rank1) {
    for (int l0 = 0; l0 < n_layers && !dry; l0 += RANK1_MAX_LAYERS) {
      const int cnt = std::min(RANK1_MAX_LAYERS, n_layers - l0);
      const void *dzp[RANK1_MAX_LAYERS], *ap[RANK1_MAX_LAYERS];
      void *wp[RANK1_MAX_LAYERS], *bp[RANK1_MAX_LAYERS];
      int64_t rows[RANK1_MAX_LAYERS], cols[RANK1_MAX_LAYERS];
      for (int q = 0; q < cnt; ++q) {
        const int l = l0 + q;
        dzp[q] = dz[l];
        ap[q] = a_in[l];
        wp[q] = gw[l]->ptr;
        bp[q] = gb[l]->ptr;
        rows[q] = w[l]->dims[0];
        cols[q] = w[l]->dims[1];
      }
      launch_rank1_many(dt, cnt, dzp, ap, wp, bp, rows, cols, sgd ? -rate : 1.0, sgd, S());
    }
    return;
  }
  int first = n_layers - 1;
  if (n_layers >= 2 && launch_gemm_small_pair(grad(n_layers - 2), grad(n_layers - 1), S(), dry)) first = n_layers - 3;
  for (int l = first; l >= 0; --l) {
    const GemmProblem p = grad(l);
    if (gemm_small_takes(p)) {
      if (!dry) launch_gemm_small(p, S());
      continue;
    }
    TO_CHECK(dt == TO_F32, TO_ERR_UNSUPPORTED, "pre-fused fp64 path: a contraction is outside the small-GEMM range");
    if (dry) continue;
    GemmProblem q = p;
    q.rowsum = nullptr;
    launch_gemm_mfma(q, S());
    launch_sum_axis(dt, dz[l], gb[l]->ptr, 1, B, w[l]->dims[0], 0, w[l]->dims[0], 1, S());
  }
}

// A validated step on the batch of x (y: x itself for an autoencoder): operands produced, destinations claimed, launched.
static void step_on_batch(const StackStep& step, to_tensor x, to_tensor y, to_tensor losses) {
  const int n_layers = step.n_layers;
  const to_tensor *w = step.w, *b = step.b, *gw = step.gw, *gb = step.gb;
  ensure(x);
  ensure(y);
  if (losses) { ensure(losses); before_write(losses); }
  for (int l = 0; l < n_layers; ++l) { ensure(w[l]); ensure(b[l]); ensure(gw[l]); ensure(gb[l]); }
  for (int l = 0; l < n_layers; ++l) {  // (identities: sgd's parameters get a new one, grad's destinations keep theirs)
    before_write(gw[l]);
    before_write(gb[l]);
    if (step.sgd) { w[l]->id = fresh_id(); b[l]->id = fresh_id(); }
  }
  step.launch(x->ptr, y->ptr, losses ? losses->ptr : nullptr, x->batch);
}

static void fflayer_stack_impl(int n_layers, const to_tensor* w, const to_tensor* b, int hidden_act, int out_act,
                               int loss, to_tensor x, to_tensor y, const to_tensor* gw, const to_tensor* gb,
                               to_tensor losses, bool sgd, double rate) {
  require_init();
  NONNULL(w); NONNULL(b); NONNULL(x); NONNULL(y); NONNULL(gw); NONNULL(gb);
  TO_CHECK(n_layers >= 1, TO_ERR_ARG, "need at least one layer");
  for (int l = 0; l < n_layers; ++l) { NONNULL(w[l]); NONNULL(b[l]); NONNULL(gw[l]); NONNULL(gb[l]); }
  const int hk = stack_hidden_act_check(hidden_act);
  const int head_kind = stack_loss_head(out_act, loss, "fused path: ");
  TO_CHECK(x->rank == 1 && y->rank == 1 && x->batch > 0 && x->batch == y->batch, TO_ERR_SHAPE,
           "x and y must be batched vectors with the same batch, got " + shape_str(x) + " " + shape_str(y));
  TO_CHECK(x->contiguous() && y->contiguous(), TO_ERR_ARG, "x and y must be contiguous");
  const int dt = x->dtype;
  TO_CHECK(y->dtype == dt, TO_ERR_ARG, "x and y have different dtypes");
  const int64_t B = x->batch;
  const int64_t fan_in = stack_params_check(n_layers, w, b, gw, gb, dt, x->dims[0]);
  TO_CHECK(y->dims[0] == fan_in, TO_ERR_SHAPE, "y does not match the output layer");
  if (losses) TO_CHECK(losses->rank == 0 && losses->batch == B && losses->contiguous(), TO_ERR_SHAPE,
                       "losses must be a batched scalar");
  const std::vector<int> acts((size_t)n_layers, hk);
  const StackStep step{n_layers, w, b, gw, gb, acts.data(), head_kind, dt, sgd, rate};
  step.check_wgrads(B);
  step_on_batch(step, x, y, losses);
}

to_status to_fflayer_stack_grad(int n_layers, const to_tensor* w, const to_tensor* b, int hidden_act,
                                int out_act, int loss, to_tensor x, to_tensor y, const to_tensor* gw,
                                const to_tensor* gb, to_tensor losses) {
  API_BEGIN
  fflayer_stack_impl(n_layers, w, b, hidden_act, out_act, loss, x, y, gw, gb, losses, false, 0.0);
  API_END
}

to_status to_fflayer_stack_sgd(int n_layers, const to_tensor* w, const to_tensor* b, int hidden_act, int out_act,
                               int loss, to_tensor x, to_tensor y, double rate, to_tensor losses) {
  API_BEGIN
  fflayer_stack_impl(n_layers, w, b, hidden_act, out_act, loss, x, y, w, b, losses, true, rate);
  API_END
}

// ---- minibatch SGD over a resident data set: the steps of to_fflayer_stack_sgd, one per minibatch, in one call ------------
// idx given: the rows of a chunk of consecutive steps are gathered into a pool buffer by ONE launch (minibatch_stage.hip)
// and the steps run on its slabs; idx null: the steps run on views of X / Y themselves.  Every step's slab starts on a
// 16-byte boundary, like the fresh tensor a host loop's to_batch_gather hands its step: the alignment the kernels' routes
// look at.
static int64_t g_minibatch_stage_bytes = MINIBATCH_STAGE_DEFAULT;

static void minibatch_steps(const StackStep& step, to_tensor X, to_tensor Y, int64_t n_idx, const int64_t* idx, int64_t M,
                            to_tensor losses, const std::string& F);

static void minibatch_sgd_impl(int n_layers, const to_tensor* w, const to_tensor* b, int hidden_act, int out_act, int loss,
                               to_tensor X, to_tensor Y, int64_t n_idx, const int64_t* idx, int64_t M, double rate,
                               to_tensor losses) {
  const std::string F = "to_fflayer_stack_minibatch_sgd: ";
  require_init();
  no_capture("to_fflayer_stack_minibatch_sgd");
  NONNULL(w); NONNULL(b); NONNULL(X);
  TO_CHECK(n_layers >= 1, TO_ERR_ARG, F + "need at least one layer");
  TO_CHECK(n_idx >= 1 && M >= 1, TO_ERR_ARG, F + "needs at least one sample and a minibatch of at least one row");
  for (int l = 0; l < n_layers; ++l) { NONNULL(w[l]); NONNULL(b[l]); }
  const int hk = stack_hidden_act_check(hidden_act);
  const int head_kind = stack_loss_head(out_act, loss, F);
  TO_CHECK(X->rank == 1 && X->batch > 0, TO_ERR_SHAPE, F + "X must be batched vectors, got " + shape_str(X));
  TO_CHECK(X->contiguous(), TO_ERR_ARG, F + "X must be contiguous");
  const int dt = X->dtype;
  const int64_t N = X->batch, i0 = X->dims[0];
  const int64_t nL = stack_params_check(n_layers, w, b, nullptr, nullptr, dt, i0);
  const std::vector<int> acts((size_t)n_layers, hk);
  const StackStep step{n_layers, w, b, w, b, acts.data(), head_kind, dt, true, rate};
  if (Y) {
    TO_CHECK(Y->dtype == dt, TO_ERR_ARG, F + "X and Y have different dtypes");
    TO_CHECK(Y->rank == 1 && Y->dims[0] == nL && Y->batch == N, TO_ERR_SHAPE,
             F + "Y must be " + std::to_string(nL) + "-vectors of X's batch, got " + shape_str(Y));
    TO_CHECK(Y->contiguous(), TO_ERR_ARG, F + "Y must be contiguous");
  } else {
    TO_CHECK(nL == i0, TO_ERR_SHAPE, F + "without Y the target of a row is the row itself: the output layer must have X's width");
  }
  minibatch_steps(step, X, Y, n_idx, idx, M, losses, F);
}

// What the two minibatch entries share behind the validation of their stacks: X [N; i0] contiguous, Y null or [N; n_L]
// contiguous of X's dtype, n_idx >= 1, M >= 1; step: an sgd step on the stack's own parameters.
static void minibatch_steps(const StackStep& step, to_tensor X, to_tensor Y, int64_t n_idx, const int64_t* idx, int64_t M,
                            to_tensor losses, const std::string& F) {
  const int n_layers = step.n_layers, dt = step.dt;
  const to_tensor *w = step.w, *b = step.b;
  const int64_t N = X->batch, i0 = X->dims[0], nL = w[n_layers - 1]->dims[0];
  if (losses) {
    TO_CHECK(losses->dtype == dt, TO_ERR_ARG, F + "X and losses have different dtypes");
    TO_CHECK(losses->rank == 0 && losses->batch == n_idx && losses->contiguous(), TO_ERR_SHAPE,
             F + "losses must be a contiguous batched scalar of batch n_idx");
  }
  if (idx) {
    for (int64_t k = 0; k < n_idx; ++k)
      TO_CHECK(idx[k] >= 0 && idx[k] < N, TO_ERR_SHAPE, F + "sample index out of range");
  } else {
    TO_CHECK(n_idx <= N, TO_ERR_SHAPE, F + "more samples than rows");
  }
  if (M > n_idx) M = n_idx;
  const int64_t n_steps = (n_idx + M - 1) / M, tail_rows = n_idx - (n_steps - 1) * M;
  // nothing half-trained: every refusal of a step, for both batches that occur, before the first launch
  step.check_sgd(M);
  if (tail_rows != M) step.check_sgd(tail_rows);

  // ---- operands produced; destinations claimed -----------------------------------------------------------------------
  ensure(X);
  if (Y) ensure(Y);
  for (int l = 0; l < n_layers; ++l) { ensure(w[l]); ensure(b[l]); }
  if (losses) claim(losses);
  for (int l = 0; l < n_layers; ++l) {  // in-place writes: recorded readers of the old values first, new identities after
    claim(w[l]);
    claim(b[l]);
  }
  const int64_t es = dt == TO_F64 ? 8 : 4;
  auto loss_at = [&](int64_t k) -> void* { return losses ? at(losses->ptr, k * M, es) : nullptr; };
  auto rows_of = [&](int64_t k) { return k + 1 == n_steps ? tail_rows : M; };
  if (!idx) {
    for (int64_t k = 0; k < n_steps; ++k) {
      const void* x = at(X->ptr, k * M * i0, es);
      step.launch(x, Y ? at(Y->ptr, k * M * nL, es) : x, loss_at(k), rows_of(k));
    }
    return;
  }
  // the device's copy of idx: through the pinned ring up to a slot of it (nothing in this call uploads another table, so the
  // slot holds for all of its launches), beyond that the staged transfer into a pool buffer
  Holder order;
  const long long* didx;
  if ((size_t)n_idx * sizeof(int64_t) <= 65536) {
    didx = static_cast<const long long*>(table_upload(idx, (size_t)n_idx * sizeof(int64_t), S()));
  } else {
    const int64_t nl = (n_idx * 8 + 3) / 4;
    order.t = new_tensor(1, &nl, 0);
    host_to_device(order.t->ptr, idx, (size_t)n_idx * sizeof(int64_t), S());
    didx = static_cast<const long long*>(order.t->ptr);
  }
  // a chunk: consecutive steps whose slabs fit the bound, one step at least
  auto slab = [](int64_t bytes) { return (bytes + 15) / 16 * 16; };
  const int64_t x_slab = slab(M * i0 * es), y_slab = Y ? slab(M * nL * es) : 0;
  int64_t chunk = g_minibatch_stage_bytes / (x_slab + y_slab);
  chunk = std::max<int64_t>(1, std::min(chunk, n_steps));
  const int64_t stage_floats = chunk * (x_slab + y_slab) / 4;
  TO_CHECK(stage_floats <= 2147483647LL, TO_ERR_SHAPE, F + "a minibatch does not fit one stage buffer");
  Holder stage(new_tensor(1, &stage_floats, 0));
  char* const xs = static_cast<char*>(stage.t->ptr);
  char* const ys = xs + chunk * x_slab;
  for (int64_t k0 = 0; k0 < n_steps; k0 += chunk) {
    const int64_t steps = std::min(chunk, n_steps - k0), rows = std::min(steps * M, n_idx - k0 * M);
    launch_minibatch_stage(didx + k0 * M, rows, M, X->ptr, xs, i0 * es, x_slab, Y ? Y->ptr : nullptr, Y ? ys : nullptr,
                           nL * es, y_slab, (int)es, S());
    for (int64_t j = 0; j < steps; ++j) {
      const void* x = xs + j * x_slab;
      step.launch(x, Y ? ys + j * y_slab : x, loss_at(k0 + j), rows_of(k0 + j));
    }
  }
  // (one stream: the stage buffer and the index table go back to the pool behind the launches that read them)
}

to_status to_fflayer_stack_minibatch_sgd(int n_layers, const to_tensor* w, const to_tensor* b, int hidden_act, int out_act,
                                         int loss, to_tensor X, to_tensor Y_or_null, int64_t n_idx,
                                         const int64_t* idx_or_null, int64_t minibatch, double rate,
                                         to_tensor losses_or_null) {
  API_BEGIN
  minibatch_sgd_impl(n_layers, w, b, hidden_act, out_act, loss, X, Y_or_null, n_idx, idx_or_null, minibatch, rate,
                     losses_or_null);
  API_END
}

to_status to_set_minibatch_stage_bytes(int64_t bytes, int64_t* previous_or_null) {
  API_BEGIN
  TO_CHECK(bytes >= 0, TO_ERR_ARG, "to_set_minibatch_stage_bytes: a byte count, or 0 for the default");
  if (previous_or_null) *previous_or_null = g_minibatch_stage_bytes;
  g_minibatch_stage_bytes = bytes ? bytes : MINIBATCH_STAGE_DEFAULT;
  API_END
}

// ---- encoder / decoder pairs of ffLayer stacks (AutoEncoder.hs) -----------------------------------------------------------
// Layers 0 .. n_enc-1 are the encoder, n_enc .. L-1 the decoder; act[n_enc-1] = code_act (logistic, tanh or none), the head
// one of four pairs, the target of a row the row itself.  grad / sgd / minibatch_sgd are StackStep with those per-layer
// activations on (x, y = x): a uniform stack with one of the two old pairs issues to_fflayer_stack_*'s launches.
static int ae_act_kind(int act, bool identity_too, const std::string& what) {
  if (act == TO_ACT_LOGISTIC) return ACT_KIND_LOGISTIC;
  if (act == TO_ACT_TANH) return ACT_KIND_TANH;
  if (act == TO_ACT_IDENTITY && identity_too) return ACT_KIND_IDENTITY;
  fail(TO_ERR_UNSUPPORTED, what + (identity_too ? " must be logistic, tanh or identity" : " must be logistic or tanh"));
}
// stack_loss_head's numbers and, behind them, 3 = (tanh, squaredError), 4 = (identity, squaredError): launch_recon_head's pairs
static int ae_loss_head(int out_act, int loss, const std::string& F) {
  if (out_act == TO_ACT_SOFTMAX && loss == TO_LOSS_CROSS_ENTROPY) return 1;
  if (loss == TO_LOSS_SQUARED_ERROR && out_act == TO_ACT_LOGISTIC) return 2;
  if (loss == TO_LOSS_SQUARED_ERROR && out_act == TO_ACT_TANH) return 3;
  if (loss == TO_LOSS_SQUARED_ERROR && out_act == TO_ACT_IDENTITY) return 4;
  fail(TO_ERR_UNSUPPORTED, F + "(softmax, crossEntropy) or (logistic / tanh / identity, squaredError) only");
}
static std::vector<int> ae_acts(int n_enc, int n_dec, const to_tensor* w, const to_tensor* b, int hidden_act, int code_act,
                                const std::string& F) {
  NONNULL(w); NONNULL(b);
  TO_CHECK(n_enc >= 1 && n_dec >= 1, TO_ERR_ARG, F + "the encoder and the decoder need at least one layer each");
  std::vector<int> acts((size_t)(n_enc + n_dec), ae_act_kind(hidden_act, false, F + "the hidden activation"));
  acts[(size_t)n_enc - 1] = ae_act_kind(code_act, true, F + "the code activation");
  return acts;
}
// an output of the batch of `like`: n-vectors (n = 0: scalars), contiguous, of its dtype
static void ae_out_check(to_tensor t, to_tensor like, int64_t n, const std::string& F, const char* what) {
  TO_CHECK(t->dtype == like->dtype, TO_ERR_ARG, F + "x and " + what + " have different dtypes");
  TO_CHECK((n ? t->rank == 1 && t->dims[0] == n : t->rank == 0) && t->batch == like->batch, TO_ERR_SHAPE,
           F + what + " must be " + (n ? std::to_string(n) + "-vectors" : std::string("scalars")) + " of the input's batch, got " +
               shape_str(t));
  TO_CHECK(t->contiguous(), TO_ERR_ARG, F + what + " must be contiguous");
}
// run / decode write caller-allocated tensors while their inputs are still being read (recon == x would have the last GEMM
// write z over the target rows): an output may overlap neither an input, nor another output, nor a parameter
static void ae_no_alias(std::initializer_list<to_tensor> outs, to_tensor in, int n, const to_tensor* w, const to_tensor* b,
                        const std::string& F) {
  for (auto o = outs.begin(); o != outs.end(); ++o) {
    bool bad = stack_overlap(*o, in);
    for (auto q = outs.begin(); q != o; ++q) bad = bad || stack_overlap(*o, *q);
    for (int l = 0; l < n; ++l) bad = bad || stack_overlap(*o, w[l]) || stack_overlap(*o, b[l]);
    TO_CHECK(!bad, TO_ERR_ARG, F + "an output overlaps the input, another output or a parameter");
  }
}
// layers l0 .. l1-1, each with its activation; the last one into `last_out` (null: scratch).  Returns where the last one is.
static const void* ae_layers(int dt, const to_tensor* w, const to_tensor* b, const int* acts, int l0, int l1, const void* prev,
                             int64_t prev_sm, int64_t B, void* last_out, std::deque<Holder>& keep) {
  for (int l = l0; l < l1; ++l) {
    const int64_t n = w[l]->dims[0];
    void* C = last_out;
    if (l + 1 < l1 || !C) {
      keep.emplace_back(new_tensor(1, &n, B, dt));
      C = keep.back().t->ptr;
    }
    stack_layer_forward(dt, w[l], b[l], acts[l], prev, prev_sm, C, B);
    prev = C;
    prev_sm = n;
  }
  return prev;
}
// the decoder from the code rows on: its hidden layers, the last contraction into z (out itself, or scratch) and the head
static void ae_decoder(int dt, int n_enc, int L, const to_tensor* w, const to_tensor* b, const int* acts, int head,
                       const void* code, int64_t code_sm, const void* target, int64_t t_sm, void* out, void* losses, int64_t B) {
  std::deque<Holder> keep;
  const void* prev = ae_layers(dt, w, b, acts, n_enc, L - 1, code, code_sm, B, nullptr, keep);
  const to_tensor WL = w[L - 1];
  const int64_t nL = WL->dims[0], prev_sm = L - 1 > n_enc ? WL->dims[1] : code_sm;
  void* z = out;  // (the head reads each element of z before it writes the same element of out)
  if (!z) {
    keep.emplace_back(new_tensor(1, &nL, B, dt));
    z = keep.back().t->ptr;
  }
  run_gemm(row_gemm(dt, prev, prev_sm, 1, WL->ptr, 1, WL->dims[1], z, B, nL, WL->dims[1]));
  launch_recon_head(dt, head, z, b[L - 1]->ptr, target, t_sm, nullptr, out, losses, B, nL, S());
}

static void ae_run_impl(int n_enc, int n_dec, const to_tensor* w, const to_tensor* b, int hidden_act, int code_act, int out_act,
                        int loss, to_tensor x, to_tensor code, to_tensor recon, to_tensor losses) {
  const std::string F = "to_autoencoder_stack_run: ";
  require_init();
  no_capture("to_autoencoder_stack_run");
  NONNULL(x);
  const std::vector<int> acts = ae_acts(n_enc, n_dec, w, b, hidden_act, code_act, F);
  const int head = ae_loss_head(out_act, loss, F), L = n_enc + n_dec;
  TO_CHECK(code || recon || losses, TO_ERR_ARG, F + "no output asked for (code, recon or losses)");
  TO_CHECK(x->rank == 1 && x->dims[0] >= 1, TO_ERR_SHAPE, F + "x must be a (batched) vector, got " + shape_str(x));
  const int dt = x->dtype;
  const int64_t i0 = x->dims[0], B = x->batch > 0 ? x->batch : 1;
  const int64_t c = stack_params_check(n_enc, w, b, nullptr, nullptr, dt, i0);
  TO_CHECK(stack_params_check(n_dec, w + n_enc, b + n_enc, nullptr, nullptr, dt, c) == i0, TO_ERR_SHAPE,
           F + "the decoder's last layer must have x's width");
  if (code) ae_out_check(code, x, c, F, "code");
  if (recon) ae_out_check(recon, x, i0, F, "recon");
  if (losses) ae_out_check(losses, x, 0, F, "losses");
  ae_no_alias({code, recon, losses}, x, L, w, b, F);
  ensure(x);
  for (int l = 0; l < L; ++l) { ensure(w[l]); ensure(b[l]); }
  if (code) claim(code);
  if (recon) claim(recon);
  if (losses) claim(losses);
  // rows with unit element stride (a strided vector view is packed first); the rows themselves may lie anywhere
  Holder xc;
  const to_tensor xr = unit_stride_rows(x, xc);
  const int64_t x_sm = x->batch > 0 ? xr->bstride : i0;
  std::deque<Holder> keep;
  const void* cp = ae_layers(dt, w, b, acts.data(), 0, n_enc, xr->ptr, x_sm, B, code ? code->ptr : nullptr, keep);
  if (recon || losses)   // (code alone: the decoder is not run)
    ae_decoder(dt, n_enc, L, w, b, acts.data(), head, cp, c, xr->ptr, x_sm, recon ? recon->ptr : nullptr,
               losses ? losses->ptr : nullptr, B);
}

static void ae_decode_impl(int n_enc, int n_dec, const to_tensor* w, const to_tensor* b, int hidden_act, int out_act,
                           to_tensor code, to_tensor out) {
  const std::string F = "to_autoencoder_stack_decode: ";
  require_init();
  no_capture("to_autoencoder_stack_decode");
  NONNULL(code); NONNULL(out);
  const std::vector<int> acts = ae_acts(n_enc, n_dec, w, b, hidden_act, TO_ACT_IDENTITY, F);
  const int head = ae_loss_head(out_act, out_act == TO_ACT_SOFTMAX ? TO_LOSS_CROSS_ENTROPY : TO_LOSS_SQUARED_ERROR, F);
  const int L = n_enc + n_dec;
  TO_CHECK(code->rank == 1 && code->dims[0] >= 1, TO_ERR_SHAPE, F + "code must be a (batched) vector, got " + shape_str(code));
  const int dt = code->dtype;
  const int64_t c = code->dims[0], B = code->batch > 0 ? code->batch : 1;
  const int64_t nL = stack_params_check(n_dec, w + n_enc, b + n_enc, nullptr, nullptr, dt, c);
  ae_out_check(out, code, nL, F, "out");
  ae_no_alias({out}, code, n_dec, w + n_enc, b + n_enc, F);
  ensure(code);
  for (int l = n_enc; l < L; ++l) { ensure(w[l]); ensure(b[l]); }
  claim(out);
  Holder cc;
  const to_tensor cr = unit_stride_rows(code, cc);
  ae_decoder(dt, n_enc, L, w, b, acts.data(), head, cr->ptr, code->batch > 0 ? cr->bstride : c, nullptr, 0, out->ptr, nullptr, B);
}

static void ae_step_impl(const std::string& F, int n_enc, int n_dec, const to_tensor* w, const to_tensor* b, int hidden_act,
                         int code_act, int out_act, int loss, to_tensor x, const to_tensor* gw, const to_tensor* gb,
                         to_tensor losses, bool sgd, double rate) {
  require_init();
  NONNULL(x); NONNULL(gw); NONNULL(gb);
  const std::vector<int> acts = ae_acts(n_enc, n_dec, w, b, hidden_act, code_act, F);
  const int head = ae_loss_head(out_act, loss, F), L = n_enc + n_dec;
  TO_CHECK(x->rank == 1 && x->batch > 0, TO_ERR_SHAPE, F + "x must be batched vectors, got " + shape_str(x));
  TO_CHECK(x->contiguous(), TO_ERR_ARG, F + "x must be contiguous");
  const int dt = x->dtype;
  TO_CHECK(stack_params_check(L, w, b, gw, gb, dt, x->dims[0]) == x->dims[0], TO_ERR_SHAPE,
           F + "the decoder's last layer must have x's width");
  if (losses) ae_out_check(losses, x, 0, F, "losses");
  const StackStep step{L, w, b, gw, gb, acts.data(), head, dt, sgd, rate};
  step.check_step(x->batch);   // every refusal before the first launch
  step_on_batch(step, x, x, losses);
}

static void ae_minibatch_impl(int n_enc, int n_dec, const to_tensor* w, const to_tensor* b, int hidden_act, int code_act,
                              int out_act, int loss, to_tensor X, int64_t n_idx, const int64_t* idx, int64_t M, double rate,
                              to_tensor losses) {
  const std::string F = "to_autoencoder_stack_minibatch_sgd: ";
  require_init();
  no_capture("to_autoencoder_stack_minibatch_sgd");
  NONNULL(X);
  const std::vector<int> acts = ae_acts(n_enc, n_dec, w, b, hidden_act, code_act, F);
  const int head = ae_loss_head(out_act, loss, F), L = n_enc + n_dec;
  TO_CHECK(n_idx >= 1 && M >= 1, TO_ERR_ARG, F + "needs at least one sample and a minibatch of at least one row");
  TO_CHECK(X->rank == 1 && X->batch > 0, TO_ERR_SHAPE, F + "X must be batched vectors, got " + shape_str(X));
  TO_CHECK(X->contiguous(), TO_ERR_ARG, F + "X must be contiguous");
  const int dt = X->dtype;
  TO_CHECK(stack_params_check(L, w, b, nullptr, nullptr, dt, X->dims[0]) == X->dims[0], TO_ERR_SHAPE,
           F + "the decoder's last layer must have X's width");
  const StackStep step{L, w, b, w, b, acts.data(), head, dt, true, rate};
  minibatch_steps(step, X, nullptr, n_idx, idx, M, losses, F);
}

to_status to_autoencoder_stack_run(int n_enc, int n_dec, const to_tensor* w, const to_tensor* b, int hidden_act, int code_act,
                                   int out_act, int loss, to_tensor x, to_tensor code_or_null, to_tensor recon_or_null,
                                   to_tensor losses_or_null) {
  API_BEGIN
  ae_run_impl(n_enc, n_dec, w, b, hidden_act, code_act, out_act, loss, x, code_or_null, recon_or_null, losses_or_null);
  API_END
}

to_status to_autoencoder_stack_decode(int n_enc, int n_dec, const to_tensor* w, const to_tensor* b, int hidden_act, int out_act,
                                      to_tensor code, to_tensor out) {
  API_BEGIN
  ae_decode_impl(n_enc, n_dec, w, b, hidden_act, out_act, code, out);
  API_END
}

to_status to_autoencoder_stack_grad(int n_enc, int n_dec, const to_tensor* w, const to_tensor* b, int hidden_act, int code_act,
                                    int out_act, int loss, to_tensor x, const to_tensor* gw, const to_tensor* gb,
                                    to_tensor losses_or_null) {
  API_BEGIN
  ae_step_impl("to_autoencoder_stack_grad: ", n_enc, n_dec, w, b, hidden_act, code_act, out_act, loss, x, gw, gb,
               losses_or_null, false, 0.0);
  API_END
}

to_status to_autoencoder_stack_sgd(int n_enc, int n_dec, const to_tensor* w, const to_tensor* b, int hidden_act, int code_act,
                                   int out_act, int loss, to_tensor x, double rate, to_tensor losses_or_null) {
  API_BEGIN
  ae_step_impl("to_autoencoder_stack_sgd: ", n_enc, n_dec, w, b, hidden_act, code_act, out_act, loss, x, w, b, losses_or_null,
               true, rate);
  API_END
}

to_status to_autoencoder_stack_minibatch_sgd(int n_enc, int n_dec, const to_tensor* w, const to_tensor* b, int hidden_act,
                                             int code_act, int out_act, int loss, to_tensor X, int64_t n_idx,
                                             const int64_t* idx_or_null, int64_t minibatch, double rate,
                                             to_tensor losses_or_null) {
  API_BEGIN
  ae_minibatch_impl(n_enc, n_dec, w, b, hidden_act, code_act, out_act, loss, X, n_idx, idx_or_null, minibatch, rate,
                    losses_or_null);
  API_END
}

// `foldl' trainNetwork` over samples (app/MNIST.hs:390-396) of an ffLayer stack as ONE persistent launch.
static void online_sgd_impl(int n_layers, const to_tensor* w, const to_tensor* b, int hidden_act, int out_act, int loss,
                            to_tensor X, to_tensor Y, int64_t n_idx, const int64_t* idx, double rate) {
  require_init();
  no_capture("to_fflayer_stack_online_sgd");
  NONNULL(w); NONNULL(b); NONNULL(X); NONNULL(Y);
  TO_CHECK(n_layers >= 2 && n_layers <= 6, TO_ERR_UNSUPPORTED, "online SGD kernel: 2..6 layers");
  const int hk = stack_hidden_act_check(hidden_act, "online SGD kernel: ");
  const int head = stack_loss_head(out_act, loss, "online SGD kernel: ");
  TO_CHECK(X->rank == 1 && Y->rank == 1 && X->batch > 0 && X->batch == Y->batch && X->contiguous() && Y->contiguous(),
           TO_ERR_SHAPE, "X and Y must be contiguous batched vectors of one batch, got " + shape_str(X) + " " + shape_str(Y));
  const int dt = X->dtype;
  TO_CHECK(Y->dtype == dt, TO_ERR_ARG, "X and Y have different dtypes");
  TO_CHECK(n_idx >= 0, TO_ERR_ARG, "negative sample count");
  TO_CHECK(Y->dims[0] == stack_params_check(n_layers, w, b, nullptr, nullptr, dt, X->dims[0]), TO_ERR_SHAPE,
           "Y does not match the output layer");
  int64_t dims[8];
  dims[0] = X->dims[0];
  for (int l = 0; l < n_layers; ++l) dims[l + 1] = w[l]->dims[0];
  int G = 0, rpw = 0;
  size_t lds = 0;
  TO_CHECK(online_sgd_plan(dt, n_layers, dims, &G, &rpw, &lds), TO_ERR_UNSUPPORTED,
           "online SGD kernel: the stack does not fit (input <= 2048, head <= 64 outputs, 160 KiB of LDS per workgroup)");
  for (int64_t k = 0; k < n_idx; ++k)
    TO_CHECK(!idx || (idx[k] >= 0 && idx[k] < X->batch), TO_ERR_SHAPE, "sample index out of range");
  TO_CHECK(idx || n_idx <= X->batch, TO_ERR_SHAPE, "more samples than rows");
  ensure(X);
  ensure(Y);
  void *wp[6], *bp[6];
  for (int l = 0; l < n_layers; ++l) {  // in-place writes: recorded readers of the old values first, new identities after
    claim(w[l]);
    claim(b[l]);
    wp[l] = w[l]->ptr;
    bp[l] = b[l]->ptr;
  }
  if (n_idx > 0) run_online_sgd(dt, n_layers, dims, wp, bp, X, Y, idx, n_idx, rate, head, hk);
}

to_status to_fflayer_stack_online_sgd(int n_layers, const to_tensor* w, const to_tensor* b, int hidden_act, int out_act,
                                      int loss, to_tensor X, to_tensor Y, int64_t n_idx, const int64_t* idx_or_null,
                                      double rate) {
  API_BEGIN
  online_sgd_impl(n_layers, w, b, hidden_act, out_act, loss, X, Y, n_idx, idx_or_null, rate);
  API_END
}

// `runNetwork` (FeedForward.hs:123-129) of an ffLayer stack over a batch and the folds of `validate` / `confusion`
// (app/MNIST.hs:366-389).  Hidden layers: one GEMM each, bias + activation (logistic / tanh) in its epilogue where the kernel carries one,
// else a plain GEMM and one elementwise launch.  The head (infer_head.hip): n_L <= 32 the last layer's contraction and
// everything after it in one launch; wider, the last GEMM into scratch (or `out` itself) and one row launch.
static void fflayer_stack_infer_impl(int n_layers, const to_tensor* w, const to_tensor* b, int hidden_act, int out_act,
                                     to_tensor x, to_tensor y, to_tensor out, int64_t* classes, int64_t* confusion) {
  require_init();
  no_capture("to_fflayer_stack_infer");
  NONNULL(w); NONNULL(b); NONNULL(x);
  TO_CHECK(n_layers >= 1, TO_ERR_ARG, "need at least one layer");
  TO_CHECK(out || classes || confusion, TO_ERR_ARG, "infer: no output asked for (out, classes or confusion)");
  TO_CHECK(!confusion || y, TO_ERR_ARG, "infer: the confusion matrix needs the targets y");
  const int hk = stack_hidden_act_check(hidden_act);
  TO_CHECK(out_act == TO_ACT_SOFTMAX || out_act == TO_ACT_LOGISTIC, TO_ERR_UNSUPPORTED,
           "infer: the output activation must be softmax or logistic");
  TO_CHECK(x->rank == 1 && x->dims[0] >= 1, TO_ERR_SHAPE, "infer: x must be a (batched) vector, got " + shape_str(x));
  const int dt = x->dtype;
  const int64_t nL = stack_params_check(n_layers, w, b, nullptr, nullptr, dt, x->dims[0]);
  const int64_t B = x->batch > 0 ? x->batch : 1;
  if (y) {
    TO_CHECK(y->dtype == dt, TO_ERR_ARG, "infer: x and y have different dtypes");
    TO_CHECK(y->rank == 1 && y->dims[0] == nL && y->batch == x->batch, TO_ERR_SHAPE,
             "infer: y must be " + std::to_string(nL) + "-vectors of x's batch, got " + shape_str(y));
  }
  if (out) {
    TO_CHECK(out->dtype == dt, TO_ERR_ARG, "infer: x and out have different dtypes");
    TO_CHECK(out->rank == 1 && out->dims[0] == nL && out->batch == x->batch, TO_ERR_SHAPE,
             "infer: out must be " + std::to_string(nL) + "-vectors of x's batch, got " + shape_str(out));
    TO_CHECK(out->contiguous(), TO_ERR_ARG, "infer: out must be contiguous");
  }
  ensure(x);
  if (y) ensure(y);
  for (int l = 0; l < n_layers; ++l) { ensure(w[l]); ensure(b[l]); }
  if (out) claim(out);
  // rows with unit element stride (a strided vector view is packed first); the rows themselves may lie anywhere
  Holder xc, yc;
  const to_tensor xr = unit_stride_rows(x, xc), yr = unit_stride_rows(y, yc);
  const int64_t x_sm = x->batch > 0 ? xr->bstride : 0;
  const int64_t y_sm = y && y->batch > 0 ? yr->bstride : 0;
  // C[B, n] = A[B, K] . W^T : B operand element (k, j) = W[j*K + k]
  auto layer = [&](const void* A, int64_t a_sm, to_tensor W, void* C) {
    return row_gemm(dt, A, a_sm, 1, W->ptr, 1, W->dims[1], C, B, W->dims[0], W->dims[1]);
  };
  std::vector<Holder> act(n_layers);
  const void* prev = xr->ptr;
  int64_t prev_sm = x_sm;
  for (int l = 0; l + 1 < n_layers; ++l) {
    const int64_t n = w[l]->dims[0];
    act[l].t = new_tensor(1, &n, B, dt);
    stack_layer_forward(dt, w[l], b[l], hk, prev, prev_sm, act[l].t->ptr, B);
    prev = act[l].t->ptr;
    prev_sm = n;
  }
  const to_tensor WL = w[n_layers - 1], bL = b[n_layers - 1];
  Holder cls, conf, z;
  if (classes) cls.t = new_tensor(1, &B, 0);  // B int32 in a float-typed pool buffer
  if (confusion) {
    const int64_t nl = nL * nL * 2;              // n_L^2 uint64
    conf.t = new_tensor(1, &nl, 0);
    TO_HIP(hipMemsetAsync(conf.t->ptr, 0, (size_t)(nL * nL) * 8, S()));
  }
  int* cls_p = cls.t ? static_cast<int*>(cls.t->ptr) : nullptr;
  auto* conf_p = conf.t ? static_cast<unsigned long long*>(conf.t->ptr) : nullptr;
  void* out_p = out ? out->ptr : nullptr;
  const void* y_p = y ? yr->ptr : nullptr;
  const bool softmax = out_act == TO_ACT_SOFTMAX;
  if (nL <= INFER_NARROW_MAX) {
    launch_infer_narrow(dt, prev, prev_sm, B, WL->dims[1], WL->ptr, bL->ptr, (int)nL, softmax, out_p, y_p, y_sm, cls_p,
                        conf_p, S());
  } else {
    void* zp = out_p;  // the row launch reads each element of z before it writes the same element of out
    if (!zp) {
      z.t = new_tensor(1, &nL, B, dt);
      zp = z.t->ptr;
    }
    run_gemm(layer(prev, prev_sm, WL, zp));
    TO_CHECK(nL <= 2147483647LL, TO_ERR_SHAPE, "infer: output layer too wide");
    launch_infer_rows(dt, zp, B, bL->ptr, (int)nL, softmax, out_p, y_p, y_sm, cls_p, conf_p, S());
  }
  if (classes) {
    std::vector<int32_t> ids((size_t)B);
    device_to_host(ids.data(), cls_p, (size_t)B * sizeof(int32_t), S());
    for (int64_t r = 0; r < B; ++r) classes[r] = ids[(size_t)r];
  }
  if (confusion) device_to_host(confusion, conf_p, (size_t)(nL * nL) * sizeof(int64_t), S());
}

to_status to_fflayer_stack_infer(int n_layers, const to_tensor* w, const to_tensor* b, int hidden_act, int out_act,
                                 to_tensor x, to_tensor y_or_null, to_tensor out_or_null, int64_t* classes_or_null,
                                 int64_t* confusion_or_null) {
  API_BEGIN
  fflayer_stack_infer_impl(n_layers, w, b, hidden_act, out_act, x, y_or_null, out_or_null, classes_or_null,
                           confusion_or_null);
  API_END
}

// ---- `induceNetwork` iterated (FeedForward.hs:150-164; app/MNIST.hs:357-365: 5000 dependent steps on the input) --------
// Route A, per iteration: the forward of to_fflayer_stack_infer, launch_loss_grad_rows, the cotangents back through the
// layers and the last contraction with the step in its epilogue (x <- 1 x + (-rate) dz_1 W_1: alpha = -rate, beta = 1,
// Cin = C = x; when gx is wanted the last iteration runs the plain product as well, into gx).  Takes every valid stack; its launch count grows with iters.  Route B, persistent (induce_seq.hip): all
// iterations of all rows in ONE launch, where its plan fits (and, for a plan of several workgroups a row, where the
// placement probe holds).  Both iterate on a private copy of x; the caller's tensors are written once, at the end.
static int g_induce_persistent = 1;                       // to_set_induce_persistent: 0 per iteration, 1 auto, 2 wherever in range
static int64_t g_induce_persistent_runs = 0, g_induce_iter_runs = 0;

// The automatic rule.  NOT MEASURED YET: tools/induce_scan.py has not been run on a device for this change (see
// profiles/r08_induce_scan.txt and DESIGN.md section 3.3), so the default takes the persistent route only where its
// advantage follows from counting and needs no measurement to hold: a plan of ONE workgroup a row (no exchange, no
// placement precondition, nobody to wait for) with at most 256 rows, where every row has a workgroup of its own and an
// iteration is a handful of passes over LDS against six or more dependent launches on route A.  Plans of several
// workgroups a row (the reference's 784-300-100-10 in fp32) and longer batches stay on route A by default until the scan
// has been run and says otherwise; to_set_induce_persistent(2) forces them.
static bool induce_auto_persistent(const InduceSeqPlan& plan, int64_t B) {
  return plan.G == 1 && B <= 256;
}

static void induce_impl(int n_layers, const to_tensor* w, const to_tensor* b, int hidden_act, int out_act, int loss,
                        to_tensor x, to_tensor y, double rate, int64_t iters, to_tensor out, to_tensor gx, to_tensor losses) {
  const std::string F = "to_fflayer_stack_induce: ";
  require_init();
  no_capture("to_fflayer_stack_induce");
  NONNULL(w); NONNULL(b); NONNULL(x); NONNULL(y); NONNULL(out);
  TO_CHECK(n_layers >= 1, TO_ERR_ARG, F + "need at least one layer");
  TO_CHECK(iters >= 0, TO_ERR_ARG, F + "negative iteration count");
  TO_CHECK(!gx || iters >= 1, TO_ERR_ARG, F + "gx is the gradient of the last iteration: it needs iters >= 1");
  const int hk = stack_hidden_act_check(hidden_act);
  const int head = stack_loss_head(out_act, loss, F);
  TO_CHECK(x->rank == 1 && x->dims[0] >= 1, TO_ERR_SHAPE, F + "x must be a (batched) vector, got " + shape_str(x));
  const int dt = x->dtype;
  const int64_t i0 = x->dims[0];
  const int64_t nL = stack_params_check(n_layers, w, b, nullptr, nullptr, dt, i0);
  const int64_t B = x->batch > 0 ? x->batch : 1;
  TO_CHECK(y->dtype == dt, TO_ERR_ARG, F + "x and y have different dtypes");
  TO_CHECK(y->rank == 1 && y->dims[0] == nL && (y->batch == 0 || y->batch == x->batch), TO_ERR_SHAPE,
           F + "y must be " + std::to_string(nL) + "-vectors of x's batch (or one unbatched target), got " + shape_str(y));
  auto like_x = [&](to_tensor t, const char* what) {
    TO_CHECK(t->dtype == dt, TO_ERR_ARG, F + "x and " + what + " have different dtypes");
    TO_CHECK(t->rank == 1 && t->dims[0] == i0 && t->batch == x->batch, TO_ERR_SHAPE,
             F + what + " must have x's shape and batch, got " + shape_str(t));
    TO_CHECK(t->contiguous(), TO_ERR_ARG, F + what + " must be contiguous");
  };
  like_x(out, "out");
  if (gx) like_x(gx, "gx");
  if (losses) {
    TO_CHECK(losses->dtype == dt, TO_ERR_ARG, F + "x and losses have different dtypes");
    TO_CHECK(losses->rank == 1 && losses->dims[0] == iters && losses->batch == x->batch, TO_ERR_SHAPE,
             F + "losses must be [B; " + std::to_string(iters) + "] of x's batch, got " + shape_str(losses));
    TO_CHECK(losses->contiguous(), TO_ERR_ARG, F + "losses must be contiguous");
  }
  TO_CHECK(B <= 2147483647LL && B * i0 <= (1LL << 40), TO_ERR_SHAPE, F + "too many rows");

  // ---- operands produced; destinations claimed -----------------------------------------------------------------------
  ensure(x);
  ensure(y);
  for (int l = 0; l < n_layers; ++l) { ensure(w[l]); ensure(b[l]); }
  const int64_t es = dt == TO_F64 ? 8 : 4;
  if (iters == 0) {  // x to out bit for bit; nothing else is touched, neither route counted
    if (out != x) {
      claim(out);
      if (out->ptr != x->ptr) {
        const int64_t dd[2] = {B, i0}, ss[2] = {x->batch > 0 ? x->bstride : 0, x->strides[0]};
        launch_copy_strided(dt, x->ptr, out->ptr, 2, dd, ss, S());
      }
    }
    TO_HIP(hipStreamSynchronize(S()));
    return;
  }
  claim(out);
  if (gx) claim(gx);
  if (losses) claim(losses);

  // the private copy of x the iterations run on, contiguous [B][i0]
  const int64_t dx[2] = {B, i0};
  Holder cur(new_tensor(2, dx, 0, dt));
  {
    const int64_t ss[2] = {x->batch > 0 ? x->bstride : 0, x->strides[0]};
    launch_copy_strided(dt, x->ptr, cur.t->ptr, 2, dx, ss, S());
  }
  Holder gxs, lt;
  if (gx) gxs.t = new_tensor(2, dx, 0, dt);
  const int64_t dl[2] = {B, iters};
  if (losses) lt.t = new_tensor(2, dl, 0, dt);
  // targets with unit element stride; rows y_sm apart (0: one target for every row)
  Holder yc;
  const to_tensor yr = unit_stride_rows(y, yc);
  const int64_t y_sm = y->batch > 0 ? yr->bstride : 0;

  int64_t dims[INDUCE_MAX_LAYERS + 1] = {0};
  InduceSeqPlan plan;
  bool persistent = false;
  if (g_induce_persistent != 0 && n_layers <= INDUCE_MAX_LAYERS) {
    dims[0] = i0;
    for (int l = 0; l < n_layers; ++l) dims[l + 1] = w[l]->dims[0];
    persistent = induce_seq_plan(dt, n_layers, dims, B, iters, &plan) &&
                 (g_induce_persistent == 2 || induce_auto_persistent(plan, B)) &&
                 (plan.G == 1 || online_sgd_placement_ok(S()));   // (the exchange's precondition: one XCD's L2)
  }

  if (persistent) {
    const void *wp[INDUCE_MAX_LAYERS], *bp[INDUCE_MAX_LAYERS];
    for (int l = 0; l < n_layers; ++l) { wp[l] = w[l]->ptr; bp[l] = b[l]->ptr; }
    launch_induce_seq(dt, plan, n_layers, dims, wp, bp, cur.t->ptr, yr->ptr, y_sm, gxs.t ? gxs.t->ptr : nullptr,
                      lt.t ? lt.t->ptr : nullptr, B, iters, rate, head, hk, S());
    TO_HIP(hipStreamSynchronize(S()));   // the watchdog's verdict is read before anything of the caller's is written
    int64_t bad_row = 0;
    const int64_t bad = induce_seq_status(&bad_row);
    TO_CHECK(bad == 0, TO_ERR_HIP,
             F + "the persistent kernel gave up waiting for a workgroup at iteration " + std::to_string(bad - 1) + " of row " +
                 std::to_string(bad_row) + " (out, gx and losses are untouched)");
    g_induce_persistent_runs++;
  } else {
    // route A.  y as [B][nL] rows (launch_loss_grad_rows reads one target per row)
    Holder yt;
    const void* yp = yr->ptr;
    if (B > 1 && (y->batch == 0 || y_sm != nL)) {
      const int64_t dy[2] = {B, nL};
      yt.t = new_tensor(2, dy, 0, dt);
      if (y->batch == 0) {
        launch_bcast_axis(dt, yr->ptr, yt.t->ptr, 1, B, nL, 0, S());
      } else {
        const int64_t ss[2] = {y_sm, 1};
        launch_copy_strided(dt, yr->ptr, yt.t->ptr, 2, dy, ss, S());
      }
      yp = yt.t->ptr;
    }
    std::vector<Holder> act(n_layers), dz(n_layers);   // act[l]: [B][n_l], the last one z_L; dz[l]: the cotangent of z_l
    for (int l = 0; l < n_layers; ++l) {
      const int64_t d2[2] = {B, w[l]->dims[0]};
      act[l].t = new_tensor(2, d2, 0, dt);
      dz[l].t = new_tensor(2, d2, 0, dt);
    }
    Holder lcol;   // losses as [iters][B]: column k of the caller's [B][iters] is one contiguous run here
    if (losses) {
      const int64_t d2[2] = {iters, B};
      lcol.t = new_tensor(2, d2, 0, dt);
    }
    void* xp = cur.t->ptr;
    for (int64_t k = 0; k < iters; ++k) {
      const void* prev = xp;
      int64_t prev_n = i0;
      for (int l = 0; l < n_layers; ++l) {   // a_l = hidden_act(a_{l-1} W_l^T + b_l); the last layer: z_L
        const int64_t n = w[l]->dims[0];
        GemmProblem p = row_gemm(dt, prev, prev_n, 1, w[l]->ptr, 1, prev_n, act[l].t->ptr, B, n, prev_n);
        p.bias = b[l]->ptr;
        if (l + 1 < n_layers) p.act = hk + 1;
        gemm_with_epilogue(p);
        prev = act[l].t->ptr;
        prev_n = n;
      }
      launch_loss_grad_rows(dt, act[n_layers - 1].t->ptr, yp, dz[n_layers - 1].t->ptr, lcol.t ? at(lcol.t->ptr, k * B, es) : nullptr,
                            B, nL, loss_grad_rows_kind(head), S());
      for (int l = n_layers - 1; l > 0; --l) {   // dz_{l-1} = (dz_l W_l) (.) hidden_act'(a_{l-1})
        const int64_t n = w[l]->dims[0], m = w[l]->dims[1];
        GemmProblem q = row_gemm(dt, dz[l].t->ptr, n, 1, w[l]->ptr, m, 1, dz[l - 1].t->ptr, B, m, n);
        q.dact = act[l - 1].t->ptr;
        q.dact_kind = hk;
        gemm_with_epilogue(q);
      }
      const int64_t n1 = w[0]->dims[0];
      GemmProblem q = row_gemm(dt, dz[0].t->ptr, n1, 1, w[0]->ptr, i0, 1, xp, B, i0, n1);
      if (gx && k + 1 == iters) {
        // the plain product is wanted too: one more contraction, once a call.  The step itself is taken by the SAME launch
        // as in every other iteration (below), so that out's bits do not depend on whether gx was asked for -- an axpy
        // behind the plain product would round alpha * acc + x differently from the epilogue
        GemmProblem qg = q;
        qg.C = gxs.t->ptr;
        gemm_with_epilogue(qg);
      }
      q.alpha = -rate;   // x <- 1 x + (-rate) dz_1 W_1 in the contraction's epilogue
      q.beta = 1.0;
      q.Cin = xp;
      gemm_with_epilogue(q);
    }
    if (losses) {   // [iters][B] -> [B][iters]
      const int64_t ss[2] = {1, B};
      launch_copy_strided(dt, lcol.t->ptr, lt.t->ptr, 2, dl, ss, S());
    }
    g_induce_iter_runs++;
  }
  TO_HIP(hipMemcpyAsync(out->ptr, cur.t->ptr, (size_t)(B * i0 * es), hipMemcpyDeviceToDevice, S()));
  if (gx) TO_HIP(hipMemcpyAsync(gx->ptr, gxs.t->ptr, (size_t)(B * i0 * es), hipMemcpyDeviceToDevice, S()));
  if (losses) TO_HIP(hipMemcpyAsync(losses->ptr, lt.t->ptr, (size_t)(B * iters * es), hipMemcpyDeviceToDevice, S()));
  TO_HIP(hipStreamSynchronize(S()));
}

to_status to_fflayer_stack_induce(int n_layers, const to_tensor* w, const to_tensor* b, int hidden_act, int out_act,
                                  int loss, to_tensor x, to_tensor y, double rate, int64_t iters, to_tensor out,
                                  to_tensor gx_or_null, to_tensor losses_or_null) {
  API_BEGIN
  induce_impl(n_layers, w, b, hidden_act, out_act, loss, x, y, rate, iters, out, gx_or_null, losses_or_null);
  API_END
}

to_status to_set_induce_persistent(int on, int* previous_or_null) {
  API_BEGIN
  TO_CHECK(on >= 0 && on <= 2, TO_ERR_ARG,
           "to_set_induce_persistent: 0 (per iteration), 1 (automatic) or 2 (wherever in range)");
  if (previous_or_null) *previous_or_null = g_induce_persistent;
  g_induce_persistent = on;
  API_END
}

to_status to_induce_stats(int64_t* persistent_runs, int64_t* per_iteration_runs) {
  API_BEGIN
  if (persistent_runs) *persistent_runs = g_induce_persistent_runs;
  if (per_iteration_runs) *per_iteration_runs = g_induce_iter_runs;
  API_END
}

// The plans of the two persistent kernels as the entries above would get them: online_sgd_plan / induce_seq_plan themselves,
// and the placement probe's verdict.  Launches nothing but that probe (once a process).
to_status to_persist_plan_query(int kernel, int dtype, int n_layers, const int64_t* dims, int64_t B, int64_t iters,
                                int* exists, int* G, int* slice, int* last_slice, int64_t* lds_bytes, int64_t* grid,
                                int* placement_ok) {
  API_BEGIN
  require_init();
  NONNULL(dims); NONNULL(exists); NONNULL(G); NONNULL(slice); NONNULL(last_slice); NONNULL(lds_bytes); NONNULL(grid);
  NONNULL(placement_ok);
  TO_CHECK(kernel == TO_PERSIST_ONLINE_SGD || kernel == TO_PERSIST_INDUCE, TO_ERR_ARG, "persist_plan_query: unknown kernel");
  TO_CHECK(dtype == TO_F32 || dtype == TO_F64, TO_ERR_ARG, "unknown dtype");
  TO_CHECK(n_layers >= 1 && n_layers <= 7, TO_ERR_ARG, "persist_plan_query: 1..7 layers (dims holds n_layers + 1 widths)");
  int g = 0, sl = 0, last = 0;
  int64_t lds = 0, gr = 0;
  bool ok;
  if (kernel == TO_PERSIST_ONLINE_SGD) {
    size_t l = 0;
    ok = online_sgd_plan(dtype, n_layers, dims, &g, &sl, &l);
    if (ok) {
      lds = (int64_t)l;
      gr = 8 * g;
      last = (int)(dims[1] - (int64_t)(g - 1) * sl);
    }
  } else {
    InduceSeqPlan plan;
    ok = induce_seq_plan(dtype, n_layers, dims, B, iters, &plan);
    if (ok) {
      g = plan.G;
      sl = plan.cw;
      lds = (int64_t)plan.lds;
      gr = plan.grid;
      last = (int)(dims[0] - (int64_t)(g - 1) * sl);
    }
  }
  const bool placed = online_sgd_placement_ok(S());
  *exists = ok ? 1 : 0;
  *G = ok ? g : 0;
  *slice = ok ? sl : 0;
  *last_slice = ok ? last : 0;
  *lds_bytes = lds;
  *grid = gr;
  *placement_ok = placed ? 1 : 0;
  API_END
}

}  // extern "C"
