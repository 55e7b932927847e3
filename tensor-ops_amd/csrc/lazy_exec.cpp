// Execution of one planned flush of the recorded class-method stream (lazy.cpp), and the step description.  The plan is
// read-only here: what has run, what has storage, what landed in its destination -- and which forwarding decisions
// survived a group falling apart at run time -- is Exec's own state.
#include "lazy_plan.hpp"

namespace to {

static std::vector<StepDesc>* g_describe = nullptr;
void lazy_describe_into(std::vector<StepDesc>* v) { g_describe = v; }
static void describe_gemm(const GemmProblem& p) {
  if (!g_describe) return;
  StepDesc d;
  d.kind = 0;
  d.p = p;
  g_describe->push_back(d);
}
void describe_other() {
  if (!g_describe) return;
  StepDesc d;
  d.kind = 2;
  g_describe->push_back(d);
}

struct Exec {
  const Plan& pl;
  std::vector<char> done;               // per group: it has run (alone, or as part of a pair, a unit or a batch)
  std::vector<char> has_storage, copied;  // per node: storage was produced by this flush / it was produced in its destination
  std::vector<char> fwd;                // per node: the plan's forwarding decisions that still hold (run_members gives one up)
  std::vector<to_tensor> finish;  // handles whose value now exists: their nodes are dropped at the end
  const char* why = "";
  explicit Exec(const Plan& p)
      : pl(p), done(p.d.gs.size(), 0), has_storage(p.ns.size(), 0), copied(p.ns.size(), 0), fwd(p.d.fwd) {}

  void in_ready(const Node* n) {
    for (to_tensor x : n->in) {
      if (!x->ptr) resolve_view(x);
      TO_CHECK(x->ptr != nullptr, TO_ERR_STATE, "internal: input of a recorded op was not produced first");
    }
  }
  void stored(int i) {
    if (has_storage[i]) return;
    has_storage[i] = 1;
    finish.push_back(pl.ns[i].h);
  }

  // one recorded op through the eager implementation
  void run_single(int i) {
    const PN& pn = pl.ns[i];
    if (has_storage[i] || pn.h->ptr) return;
    Node* n = pn.n;
    in_ready(n);
    describe_other();
    Holder r;
    switch (n->d.op) {
      case N_GMUL: r.t = gmul_impl(n->d.lm, n->d.lo, n->d.ln, n->in[0], n->in[1], n->d.reduce); break;
      case N_LIFT: r.t = lift_impl(n->d.f, (int)n->in.size(), n->in.data(), 0, nullptr); break;
      case N_DACT: r.t = kind_impl(n->d.lm ? EW_MUL_1MH2 : EW_MUL_H1MH, 2, n->in.data()); break;
      case N_SUM: r.t = sum_impl((int)n->in.size(), n->in.data(), pn.h->rank, pn.h->dims, pn.h->dtype); break;
      case N_SCALE: r.t = affine_impl(1, n->in.data(), &n->d.alpha, 0.0); break;
      case N_SUM_ROWS: r.t = sum_rows_impl(n->in[0]); break;
      case N_MAP_ROWS: r.t = map_rows_const_impl(n->d.len_n, n->in[0], pn.h); break;
      case N_BATCH_SUM: r.t = batch_sum_impl(n->in[0]); break;
      case N_STACK: r.t = stack_impl(n->d.len_n, pn.h->dims, n->in.data()); break;
      case N_FILL:
        alloc_storage(pn.h);
        launch_fill(pn.h->dtype, pn.h->ptr, pn.h->total(), n->d.alpha, S());
        stored(i);
        return;
      default: fail(TO_ERR_STATE, "internal: unknown recorded op");
    }
    if (!r.t->contiguous() || r.t->batch != pn.h->batch) {
      // (sum of one operand / batch_sum of an unbatched value return their argument: give the handle the
      //  contiguous layout it promised)
      Holder c(contiguous(r.t));
      TO_CHECK(c.t->batch == pn.h->batch, TO_ERR_STATE, "internal: result batch differs from the recorded shape");
      adopt_storage(pn.h, c.t);
    } else {
      adopt_storage(pn.h, r.t);
    }
    stored(i);
  }

  void run_members(const Gr& g) {
    if (debug_on() && g.mem.size() > 1) std::fprintf(stderr, "[lazy] group of n%d: NOT fused (%s), running %zu ops one by one\n", g.anchor, why, g.mem.size());
    for (int m : g.mem) {
      fwd[m] = 0;
      run_single(m);
    }
  }

  struct Launch {
    GemmProblem p;
    GmulPlan gp;  // keeps packed operands alive
  };

  // build the fused problem of a GEMM group; false = the kernels cannot take it as planned
  bool build(const Gr& g, Launch& L) {
    const PN& an = pl.ns[g.anchor];
    Node* n = an.n;
    for (int m : g.mem)
      if (!pl.ns[m].is_const) {
        // inputs produced inside the group do not exist (that is the point); everything else must
        for (size_t k = 0; k < pl.ns[m].n->in.size(); ++k) {
          const int q = pl.ns[m].prod[k];
          if (q >= 0 && pl.d.group[q] == pl.d.group[m] && !has_storage[q]) continue;
          to_tensor x = pl.ns[m].n->in[k];
          if (!x->ptr) resolve_view(x);
          TO_CHECK(x->ptr != nullptr, TO_ERR_STATE, "internal: input of a fused group was not produced first");
        }
      }
    // The real plan may LAUNCH (a pack of a non-collapsible operand, the pre-sum of a batch-reduced one).  An operand
    // produced by a launch that is still held back in `queue` has storage but no contents yet: issue the queue first.
    if (!queue.empty()) {
      GmulPlan dry;
      dry_plan(n, dry);
      bool from_queue = false;
      for (size_t k = 0; k < an.prod.size(); ++k) from_queue = from_queue || (an.prod[k] >= 0 && in_queue(an.prod[k]));
      if (!dry.exact && from_queue) drain();
    }
    gmul_plan(L.gp, n->d.lm, n->d.lo, n->d.ln, n->in[0], n->in[1], n->d.reduce, false);
    why = "empty contraction";
    if (L.gp.zero) return false;
    GemmProblem& p = L.p;
    p = L.gp.p;
    const bool epi = g.mem.size() > 1;
    why = "batched GEMM form";
    if (epi && (p.batch != 1 || p.reduce_batch)) return false;
    p.alpha = g.alpha;
    const to_tensor cin = operand(pl, g.cin), bias = operand(pl, g.bias), dact = operand(pl, g.dact);
    p.beta = cin ? g.beta : 0.0;
    p.Cin = cin ? cin->ptr : nullptr;
    p.bias = bias ? bias->ptr : nullptr;
    why = "bias does not run along the columns";
    if (bias && (p.N != bias->dims[0] || p.c_sm != p.N)) return false;
    p.act = g.act;
    p.dact = dact ? dact->ptr : nullptr;
    p.dact_kind = g.dact_kind;
    const bool needs_small = g.rs >= 0 || g.loss_kind != 0;
    why = "outside the small-GEMM range";
    if (needs_small && !gemm_small_route(p)) return false;
    why = "no kernel with a fused epilogue for this shape";
    if (epi && !needs_small && !gemm_epilogue_ok(p)) return false;
    if (g.loss_kind) {
      why = "loss head does not fit the kernel";
      if (!gemm_small_fuses_loss(p)) return false;
      p.loss_rows = g.loss_kind;
      p.target = operand(pl, g.target)->ptr;
      if (g.tail >= 0) {
        const int64_t tn = pl.ns[g.tail].h->dims[0];
        if (!gemm_small_fuses_tail(p, tn)) return false;
        p.tail_w = operand(pl, g.tail_w)->ptr;
        p.tail_h = operand(pl, g.tail_h)->ptr;
        p.tail_n = (int)tn;
      }
    }
    return true;
  }

  void* out_ptr(int i) {
    const PN& pn = pl.ns[i];
    if (fwd[i]) return pn.copy_dst->ptr;  // produced in place: the handle itself stays deferred
    if (!pn.h->ptr) alloc_storage(pn.h);
    return pn.h->ptr;
  }

  void bind_outputs(const Gr& g, Launch& L) {
    GemmProblem& p = L.p;
    p.C = out_ptr(g.out);
    if (g.rs >= 0) {
      p.rowsum = out_ptr(g.rs);
      if (g.rs_in) {
        p.rowsum_acc = true;
        p.rowsum_in = operand(pl, g.rs_in)->ptr;
        p.rowsum_alpha = g.rs_alpha;
      }
    }
    if (g.loss_node >= 0) p.loss_out = out_ptr(g.loss_node);
    if (g.tail >= 0) p.tail_out = out_ptr(g.tail);
  }

  void mark_outputs(const Gr& g) {
    const int outs[4] = {g.out, g.rs, g.loss_node, g.tail};
    for (int o : outs)
      if (o >= 0) {
        if (fwd[o]) copied[o] = 1;
        else stored(o);
      }
    if (g.mem.size() > 1) g_lazy_stats[1]++;
    for (int m : g.mem)
      if (m != g.out && m != g.rs && m != g.loss_node && m != g.tail) g_lazy_stats[2]++;
  }

  void launch_one(const Gr& g, Launch& L) {
    describe_gemm(L.p);
    if (g.mem.size() > 1) run_gemm_small_first(L.p);
    else run_gemm(L.p);
  }

  // Small-GEMM launches are held back for a moment: three in a row -- a forward launch, the output layer with
  // its loss head, the pair of weight gradients -- are the batched training step, which goes out as ONE launch
  // with grid barriers (gemm_small_chain_kernel) when its shapes pick the configurations that kernel is built from.
  struct Queued {
    std::unique_ptr<Launch> a, b;  // b: the second problem of a pair
    const Gr *ga = nullptr, *gb = nullptr;
  };
  std::vector<Queued> queue;

  // is PN i an output of a launch that has been planned but not issued yet?
  bool in_queue(int i) const {
    for (const Queued& e : queue)
      for (const Gr* g : {e.ga, e.gb})
        if (g && (i == g->out || i == g->rs || i == g->loss_node || i == g->tail)) return true;
    return false;
  }

  void drain() {
    if (queue.empty()) return;
    std::vector<Queued> q;
    q.swap(queue);
    for (Queued& e : q) {
      describe_gemm(e.a->p);
      if (e.b) describe_gemm(e.b->p);
    }
    if (q.size() == 3 && !q[0].b && !q[1].b && q[2].b && q[1].a->p.loss_rows && !q[0].a->p.loss_rows &&
        (launch_gemm_small_chain(q[0].a->p, q[1].a->p, q[2].a->p, q[2].b->p, S()) ||
         launch_gemm_small_chain(q[0].a->p, q[1].a->p, q[2].b->p, q[2].a->p, S()))) {
      g_lazy_stats[1] -= 2;  // one launch, not three
      return;
    }
    for (size_t qi = 0; qi < q.size(); ++qi) {
      Queued& e = q[qi];
      // a forward layer directly followed by the loss-head launch that reads its output: one launch, joined inside
      // each XCD (gemm_small_seam_kernel); the pair kernel's refusal costs nothing
      if (!e.b && qi + 1 < q.size() && !q[qi + 1].b && q[qi + 1].a->p.loss_rows && !e.a->p.loss_rows &&
          launch_gemm_small_seam(e.a->p, q[qi + 1].a->p, S())) {
        g_lazy_stats[1]--;  // one launch, not two
        ++qi;
        continue;
      }
      if (e.b) {
        if (launch_gemm_small_pair(e.a->p, e.b->p, S()) || launch_gemm_small_pair(e.b->p, e.a->p, S())) continue;
        launch_gemm_small(e.a->p, S());
        launch_gemm_small(e.b->p, S());
        g_lazy_stats[1]++;
      } else {
        launch_gemm_small(e.a->p, S());
      }
    }
  }

  void run_gemm_group(const Gr& g) {
    std::unique_ptr<Launch> L(new Launch());
    if (!build(g, *L)) {
      drain();
      run_members(g);
      return;
    }
    bind_outputs(g, *L);
    if (g.mem.size() > 1 && gemm_small_route(L->p)) {
      Queued e;
      e.a = std::move(L);
      e.ga = &g;
      queue.push_back(std::move(e));
    } else {
      drain();
      describe_gemm(L->p);
      run_gemm(L->p);
    }
    mark_outputs(g);
  }

  void run_pair(const Gr& g1, const Gr& g2) {
    std::unique_ptr<Launch> L1(new Launch()), L2(new Launch());
    const bool ok1 = build(g1, *L1), ok2 = build(g2, *L2);
    if (ok1) bind_outputs(g1, *L1);
    if (ok2) bind_outputs(g2, *L2);
    if (ok1 && ok2 && gemm_small_route(L1->p) && gemm_small_route(L2->p)) {
      Queued e;
      e.a = std::move(L1);
      e.b = std::move(L2);
      e.ga = &g1;
      e.gb = &g2;
      queue.push_back(std::move(e));
      mark_outputs(g1);
      mark_outputs(g2);
      g_lazy_stats[1]--;  // one launch, not two (drain() corrects this if the pair kernel refuses the shapes)
      return;
    }
    drain();
    if (ok1) { launch_one(g1, *L1); mark_outputs(g1); } else run_members(g1);
    if (ok2) { launch_one(g2, *L2); mark_outputs(g2); } else run_members(g2);
  }

  // all outer-product weight gradients of a one-sample step in one launch
  void run_rank1_unit(const std::vector<int>& members) {
    std::vector<std::unique_ptr<Launch>> L;
    bool ok = true;
    for (int gi : members) {
      L.emplace_back(new Launch());
      ok = ok && build(pl.d.gs[gi], *L.back());
      const GemmProblem& p = L.back()->p;
      // (a one-row / one-column operand has no stride to speak of: the output layer of tensor-ops-dots is 1 x 8)
      ok = ok && p.K == 1 && p.batch == 1 && (p.a_sm == 1 || p.M == 1) && (p.b_sn == 1 || p.N == 1) &&
           (p.beta == 0.0 || p.beta == 1.0) &&
           p.c_sm == p.N;
    }
    drain();
    if (!ok) {
      for (int gi : members) run_gemm_group(pl.d.gs[gi]);
      return;
    }
    const void *dz[RANK1_MAX_LAYERS], *a[RANK1_MAX_LAYERS], *w_in[RANK1_MAX_LAYERS], *b_in[RANK1_MAX_LAYERS];
    void *w[RANK1_MAX_LAYERS], *b[RANK1_MAX_LAYERS];
    double alpha[RANK1_MAX_LAYERS];
    int64_t rows[RANK1_MAX_LAYERS], cols[RANK1_MAX_LAYERS];
    for (size_t k = 0; k < members.size(); ++k) {
      const Gr& g = pl.d.gs[members[k]];
      bind_outputs(g, *L[k]);
      const GemmProblem& p = L[k]->p;
      dz[k] = p.A; a[k] = p.B; w[k] = p.C;
      w_in[k] = p.beta == 1.0 ? p.Cin : nullptr;
      b[k] = p.rowsum;
      b_in[k] = p.rowsum_acc ? p.rowsum_in : nullptr;
      alpha[k] = p.alpha;
      // (the bias update carries its own factor; the kernel has one per layer: they are the same -rate in every
      //  network the DSL can build, and a mismatch falls back below)
      if (p.rowsum && (p.rowsum_acc ? p.rowsum_alpha : 1.0) != p.alpha) ok = false;
      rows[k] = p.M; cols[k] = p.N;
    }
    if (!ok) {
      for (size_t k = 0; k < members.size(); ++k) { launch_one(pl.d.gs[members[k]], *L[k]); mark_outputs(pl.d.gs[members[k]]); }
      return;
    }
    if (g_describe) {
      StepDesc d;
      d.kind = 1;
      d.n = (int)members.size();
      d.p.dtype = L[0]->p.dtype;
      for (int k = 0; k < d.n; ++k) {
        d.dz[k] = dz[k]; d.a[k] = a[k]; d.w[k] = w[k]; d.b[k] = b[k]; d.w_in[k] = w_in[k]; d.b_in[k] = b_in[k];
        d.alpha[k] = alpha[k]; d.rows[k] = rows[k]; d.cols[k] = cols[k];
      }
      g_describe->push_back(d);
    }
    launch_rank1_general(L[0]->p.dtype, (int)members.size(), dz, a, w, b, w_in, b_in, alpha, rows, cols, S());
    for (int gi : members) mark_outputs(pl.d.gs[gi]);
    g_lazy_stats[1] -= (int64_t)members.size() - 1;
  }

  // a row-local subgraph as one compiled kernel (or, without a run-time compiler, op by op)
  void run_rowprog(const Gr& g) {
    RowProg& rp = *g.rowprog;
    to_tensor root = pl.ns[g.rp_root].h;
    if (!root->ptr) resolve_view(root);
    bool ok = root->ptr && root->contiguous() && rowprog_build(rp);
    const void* ext[4] = {nullptr, nullptr, nullptr, nullptr};
    for (size_t i = 0; i < g.rp_ext.size(); ++i) {
      to_tensor e = operand(pl, g.rp_ext[i]);
      if (e && !e->ptr) resolve_view(e);  // (a peer's output: produced earlier in this plan)
      ok = ok && e && e->ptr && e->contiguous();
      if (ok) ext[i] = e->ptr;
    }
    if (!ok) {
      why = rp.err.empty() ? "row program: operands not ready" : rp.err.c_str();
      run_members(g);
      return;
    }
    void* outs[4] = {nullptr, nullptr, nullptr, nullptr};
    for (size_t i = 0; i < g.rp_outs.size(); ++i) {
      const PN& on = pl.ns[g.rp_outs[i]];
      if (!on.h->ptr) alloc_storage(on.h);
      outs[i] = on.h->ptr;
    }
    describe_other();
    rowprog_launch(rp, root->ptr, ext, outs, root->batch > 0 ? root->batch : 1, S());
    for (int o : g.rp_outs) stored(o);
    g_lazy_stats[1]++;
    for (int m : g.mem)
      if (std::find(g.rp_outs.begin(), g.rp_outs.end(), m) == g.rp_outs.end()) g_lazy_stats[2]++;
  }

  // ---- sibling batches (round 6) ------------------------------------------------------------------------------------------
  // The reference's BTensor maps a GEMM over the trailing matrices of a rank > 2 operand (`mapBTM`, BTensor.hs:703-710) and a
  // `liftB` over every leaf (:345-369): through the inner boundary config 5 arrives as 512 `gemm` calls that share B and 512
  // `liftB` calls that share a closure (README.md:150-154 prescribes exactly this integration) -- 1,024 launches for what the
  // outer boundary does in two.  Deferral fuses a value with its consumers (vertically); siblings it has to find here:
  //  * plain products (no epilogue) of equal shape with the same right operand, in the range of the short-K streaming kernel
  //    once their rows are counted together: ONE launch, the A operands through a device table of pointers, the results in
  //    consecutive slices of one allocation;
  //  * lifts of the same closure whose operands lie one behind the other in memory (which is how the launch above leaves
  //    them): ONE launch over the whole range, results again in one allocation.
  // A batch runs at the place of its first member in the plan's order, so every member's inputs must have been produced by
  // then (its group's dependencies all lie earlier).  Whatever does not qualify runs as before.  Not while a step is being
  // captured or described (a table upload is no kernel launch; the step recognisers read single launches).
  static bool batching_on() {
    static const bool v = [] { const char* e = getenv("TOPS_SIBLING_BATCH"); return !(e && e[0] == '0'); }();
    return v;
  }
  std::vector<int> pos;   // group -> its place in the order (filled by run_all for plans worth looking at)

  bool deps_before(const Gr& g, int k) const {
    for (int d : g.deps)
      if (pos[(size_t)d] >= k) return false;
    return true;
  }
  bool plain_single(int gi) const {
    const Gr& g = pl.d.gs[(size_t)gi];
    return !done[gi] && g.mem.size() == 1 && g.pair < 0 && g.r1 < 0 && !g.rowprog && !fwd[g.mem[0]] && !has_storage[g.mem[0]] &&
           !pl.ns[g.mem[0]].h->ptr && !pl.ns[g.mem[0]].is_const;
  }
  // a product alone, or with nothing but an activation (and a scale) fused behind it: what the short-K kernel's epilogue carries
  bool product_family_member(int gi) const {
    const Gr& g = pl.d.gs[(size_t)gi];
    if (!g.gemm || done[gi] || g.pair >= 0 || g.r1 >= 0 || g.rowprog || g.mem.size() > 3) return false;
    if (g.rs >= 0 || g.loss_kind || g.tail >= 0 || g.bias || g.cin || g.dact || g.act > 1) return false;
    const PN& o = pl.ns[g.out];
    return !fwd[g.out] && !has_storage[g.out] && !o.h->ptr && !o.is_const && !pl.ns[g.anchor].n->d.reduce;
  }
  static bool same_epilogue(const Gr& a, const Gr& b) { return a.act == b.act && a.alpha == b.alpha && a.mem.size() == b.mem.size(); }

  bool try_gemm_batch(const std::vector<int>& order, int k) {
    const Gr& g0 = pl.d.gs[order[(size_t)k]];
    if (!product_family_member(order[(size_t)k])) return false;
    std::unique_ptr<Launch> L0(new Launch());
    if (!build(g0, *L0)) return false;
    const GemmProblem& p0 = L0->p;
    if (p0.dtype != TO_F32 || p0.batch != 1 || p0.reduce_batch || p0.beta != 0.0 || p0.bias || p0.act > 1 || p0.dact ||
        p0.a_sk != 1 || p0.M % 32 != 0 || (p0.M * p0.N * 4) % 16 != 0 || (reinterpret_cast<uintptr_t>(p0.A) & 15u))
      return false;
    std::vector<int> mem{order[(size_t)k]};
    std::vector<const void*> atab{p0.A};
    std::vector<std::unique_ptr<Launch>> keep;   // (packed operands stay alive until the launch is enqueued)
    for (size_t j = (size_t)k + 1; j < order.size() && atab.size() < 4096; ++j) {
      const Gr& g = pl.d.gs[order[j]];
      if (!product_family_member(order[j]) || !same_epilogue(g, g0) || !deps_before(g, k)) continue;
      const Node* n = pl.ns[g.anchor].n;
      const Node* n0 = pl.ns[g0.anchor].n;
      if (n->in[1] != n0->in[1] || n->d.lm != n0->d.lm || n->d.lo != n0->d.lo || n->d.ln != n0->d.ln) continue;   // (the same B handle)
      // the common case without a plan of its own: a left operand with storage and exactly the first one's layout gives the
      // first one's problem with another A (512 full plans were a third of this flush's time on the host)
      {
        to_tensor a = n->in[0], a0 = n0->in[0];
        if (a->ptr && a0->ptr && a0->ptr == p0.A && a->dtype == a0->dtype && a->batch == a0->batch && a->bstride == a0->bstride &&
            same_shape(a, a0) && std::equal(a->strides, a->strides + a->rank, a0->strides) && !(reinterpret_cast<uintptr_t>(a->ptr) & 15u) &&
            same_shape(pl.ns[g.out].h, pl.ns[g0.out].h) && pl.ns[g.out].h->batch == pl.ns[g0.out].h->batch) {
          mem.push_back(order[j]);
          atab.push_back(a->ptr);
          continue;
        }
      }
      std::unique_ptr<Launch> L(new Launch());
      if (!build(g, *L)) continue;
      const GemmProblem& p = L->p;
      if (p.dtype != p0.dtype || p.B != p0.B || p.b_sk != p0.b_sk || p.b_sn != p0.b_sn || p.M != p0.M || p.N != p0.N || p.K != p0.K ||
          p.a_sm != p0.a_sm || p.a_sk != 1 || p.batch != 1 || p.reduce_batch || p.alpha != p0.alpha || p.beta != 0.0 || p.act != p0.act ||
          p.bias || p.dact || (reinterpret_cast<uintptr_t>(p.A) & 15u))
        continue;
      mem.push_back(order[j]);
      atab.push_back(p.A);
      keep.push_back(std::move(L));
    }
    if (mem.size() < 2) return false;
    GemmProblem all = p0;
    all.M = p0.M * (int64_t)mem.size();
    all.c_sm = p0.N;
    all.C = reinterpret_cast<void*>(16);   // (placeholder with the alignment the result will have: the applicability test reads it)
    if (!gemm_skinnyk_applicable(all)) return false;
    drain();
    std::vector<to_tensor> outs;
    for (int gi : mem) outs.push_back(pl.ns[pl.d.gs[gi].out].h);
    alloc_storage_shared((int)outs.size(), outs.data());
    all.C = outs[0]->ptr;
    all.a_table = table_upload(atab.data(), atab.size() * sizeof(void*), S());
    all.a_table_rows = p0.M;
    describe_gemm(all);
    launch_gemm_skinnyk(all, S());
    for (int gi : mem) {
      done[gi] = 1;
      mark_outputs(pl.d.gs[gi]);   // (the output exists; what was fused behind the product is counted as elided)
    }
    if (debug_on()) std::fprintf(stderr, "[lazy] sibling batch: %zu products %lld x %lld x %lld with one right operand -> one launch\n", mem.size(),
                                 (long long)p0.M, (long long)p0.K, (long long)p0.N);
    return true;
  }

  bool try_lift_batch(const std::vector<int>& order, int k) {
    const Gr& g0 = pl.d.gs[order[(size_t)k]];
    if (g0.gemm || !plain_single(order[(size_t)k])) return false;
    const int i0 = g0.mem[0];
    const Node* n0 = pl.ns[i0].n;
    if (n0->d.op != N_LIFT || n0->in.empty() || n0->in.size() > 8) return false;
    to_tensor h0 = pl.ns[i0].h;
    const int64_t total = h0->total();
    const size_t bytes = (size_t)total * h0->esize();
    if (total == 0 || bytes % 16 != 0) return false;
    auto operands_ok = [&](const Node* n, to_tensor h) {
      if (n->d.op != N_LIFT || n->d.f != n0->d.f || n->in.size() != n0->in.size() || h->dtype != h0->dtype || h->total() != total ||
          h->batch != h0->batch || !same_shape(h, h0))
        return false;
      for (to_tensor x : n->in) {
        if (!x->ptr) resolve_view(x);
        if (!x->ptr || !x->contiguous() || x->total() != total || x->dtype != h0->dtype) return false;   // (no broadcast operand)
      }
      return true;
    };
    if (!operands_ok(n0, h0)) return false;
    std::vector<int> mem{order[(size_t)k]};
    for (size_t j = (size_t)k + 1; j < order.size(); ++j) {
      const Gr& g = pl.d.gs[order[j]];
      if (g.gemm || !plain_single(order[j]) || !deps_before(g, k)) continue;
      if (!operands_ok(pl.ns[g.mem[0]].n, pl.ns[g.mem[0]].h)) continue;
      mem.push_back(order[j]);
    }
    if (mem.size() < 2) return false;
    // in the order of their first operand's address; every operand then has to advance by one tensor per member
    std::sort(mem.begin(), mem.end(), [&](int a, int b) {
      return pl.ns[pl.d.gs[a].mem[0]].n->in[0]->ptr < pl.ns[pl.d.gs[b].mem[0]].n->in[0]->ptr;
    });
    const Node* nf = pl.ns[pl.d.gs[mem[0]].mem[0]].n;
    // the longest run from the front that is consecutive in every operand (what does not belong runs on its own later)
    size_t run = 1;
    for (; run < mem.size(); ++run) {
      const Node* n = pl.ns[pl.d.gs[mem[run]].mem[0]].n;
      bool ok = true;
      for (size_t q = 0; q < nf->in.size() && ok; ++q)
        ok = static_cast<const char*>(n->in[q]->ptr) == static_cast<const char*>(nf->in[q]->ptr) + run * bytes;
      if (!ok) break;
    }
    // (the run has to contain the group whose turn it is: it is the one that must be done when this returns)
    bool has_k = false;
    for (size_t r = 0; r < run; ++r) has_k = has_k || mem[r] == order[(size_t)k];
    if (run < 2 || !has_k) return false;
    mem.resize(run);
    drain();
    std::vector<to_tensor> outs;
    for (int gi : mem) outs.push_back(pl.ns[pl.d.gs[gi].mem[0]].h);
    alloc_storage_shared((int)outs.size(), outs.data());
    const void* xs[8];
    for (size_t q = 0; q < nf->in.size(); ++q) xs[q] = nf->in[q]->ptr;
    describe_other();
    lift_launch_raw(nf->d.f, (int)nf->in.size(), xs, outs[0]->ptr, total * (int64_t)run, h0->dtype);
    for (int gi : mem) {
      done[gi] = 1;
      stored(pl.d.gs[gi].mem[0]);
    }
    if (debug_on()) std::fprintf(stderr, "[lazy] sibling batch: %zu lifts of one closure over %lld elements each -> one launch\n", run, (long long)total);
    return true;
  }

  void run_all() {
    const std::vector<int>& order = pl.d.order;
    const bool look = order.size() >= 8 && batching_on() && !g_describe && !launch_recorder() && !rt().capturing;
    if (look) {
      pos.assign(pl.d.gs.size(), -1);
      for (size_t k = 0; k < order.size(); ++k) pos[(size_t)order[k]] = (int)k;
    }
    for (size_t k = 0; k < order.size(); ++k) {
      if (look && !done[order[k]] && (try_gemm_batch(order, (int)k) || try_lift_batch(order, (int)k))) continue;
      run_group(order[k]);
    }
  }

  void run_group(int gi) {
    const Gr& g = pl.d.gs[gi];
    if (done[gi]) return;
    if (g.r1 >= 0) {
      const std::vector<int>& members = pl.d.gs[g.r1].r1_members;
      for (int m : members) done[m] = 1;
      run_rank1_unit(members);
      return;
    }
    done[gi] = 1;
    if (g.pair >= 0) done[g.pair] = 1;
    if (g.rowprog) {
      drain();
      run_rowprog(g);
    } else if (!g.gemm) {
      drain();
      run_members(g);
    }
    else if (g.pair >= 0) run_pair(g, pl.d.gs[g.pair]);
    else run_gemm_group(g);
  }
};

// Runs the plan, lands what could not be produced in place, and drops the nodes of the values that exist afterwards.
void run_plan(const Plan& pl) {
  Exec ex(pl);
  std::exception_ptr err;
  try {
    ex.run_all();
    ex.drain();
    // sources that could not be produced in place: one copy launch for all of them
    std::vector<const void*> sp;
    std::vector<void*> dp;
    std::vector<int64_t> dw;
    for (size_t i = 0; i < pl.ns.size(); ++i) {
      const PN& pn = pl.ns[i];
      if (pn.copy_dst && !ex.copied[i]) {
        if (!pn.h->ptr) ex.run_single((int)i);
        if (pn.copy_dst->total() == 0) continue;
        sp.push_back(pn.h->ptr);
        dp.push_back(pn.copy_dst->ptr);
        dw.push_back(pn.copy_dst->total() * (int64_t)pn.copy_dst->esize() / 4);
      }
    }
    for (size_t b = 0; b < sp.size(); b += 16) {
      const int m = (int)std::min<size_t>(16, sp.size() - b);
      describe_other();
      launch_multi_copy(m, sp.data() + b, dp.data() + b, dw.data() + b, S());
    }
    // A result produced straight into its destination still stands for a VALUE.  If its handle is asked for later (the
    // host holds it, or an op recorded afterwards reads it) the recorded op must not run again: one of its inputs may be
    // the very destination it has just overwritten (b' = b - r g produced into b would apply the update twice).  From
    // here on the handle means "the contents of the destination": a recorded `1 * dst`, which the write hazards
    // (before_write / stale_after_write) run before dst changes again; nothing is launched unless someone asks.
    for (size_t i = 0; i < pl.ns.size(); ++i) {
      const PN& pn = pl.ns[i];
      if (!ex.fwd[i] || !ex.copied[i] || pn.h->ptr || !pn.h->node) continue;
      Node* n = pn.n;
      to_tensor d = pn.copy_dst;
      if (full_like(d, pn.h)) {
        retain_int(d);
        for (to_tensor x : n->in) release_int(x);
        n->in.assign(1, d);
        if (n->d.f) expr_release(n->d.f);
        n->d = NodeDesc{};
        n->d.op = N_SCALE;
        n->d.alpha = 1.0;
      } else {
        // (a destination of another shape, e.g. a flat parameter view: the handle gets a copy of its own -- always:
        //  even when the host has let go of it, the scope's memo table may hand it out again, and re-running its
        //  recorded op would read the destination it has just overwritten)
        alloc_storage(pn.h);
        const void* sp1 = d->ptr;
        void* dp1 = pn.h->ptr;
        int64_t dw1 = d->total() * (int64_t)d->esize() / 4;
        describe_other();
        if (d->total() > 0) launch_multi_copy(1, &sp1, &dp1, &dw1, S());
        ex.finish.push_back(pn.h);
      }
    }
  } catch (...) {
    err = std::current_exception();
    try {
      ex.drain();  // what was already planned into held-back launches still has to produce its outputs
    } catch (...) {
    }
  }
  // values that exist now no longer need their recorded op (this releases the inputs the op kept alive)
  for (to_tensor h : ex.finish) lazy_drop_node(h);
  if (err) std::rethrow_exception(err);
}
}  // namespace to
