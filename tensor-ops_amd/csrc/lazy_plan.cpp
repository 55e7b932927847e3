// The planner of one flush of the recorded class-method stream (lazy.cpp says why it exists and lists the rules): the recorded
// ops the roots depend on, the groups they fall into, forwarding into to_copy_into destinations, the order.  What it
// decides goes into the plan's Decisions record (lazy_plan.hpp) and nowhere else.
#include <cmath>
#include <cstring>
#include <unordered_map>

#include "lazy_plan.hpp"

namespace to {

// ---- the nodes of one flush -----------------------------------------------------------------------------------------------
static uint64_t g_plan_epoch = 0;

// the recorded ops the roots depend on, in recording order, with their producer / consumer links
void collect(Plan& pl, const std::vector<to_tensor>& roots) {
  pl.epoch = ++g_plan_epoch;
  std::vector<Node*> stack, all;
  auto push = [&](to_tensor t) {
    Node* p = producer(t);
    if (p && p->plan_epoch != pl.epoch) {
      p->plan_epoch = pl.epoch;
      p->plan_idx = -1;
      stack.push_back(p);
    }
  };
  for (to_tensor t : roots) push(t);
  while (!stack.empty()) {
    Node* n = stack.back();
    stack.pop_back();
    all.push_back(n);
    for (to_tensor x : n->in) push(x);
  }
  std::sort(all.begin(), all.end(), [](const Node* a, const Node* b) { return a->seq < b->seq; });
  pl.ns.resize(all.size());
  pl.d.group.assign(all.size(), -1);
  pl.d.fwd.assign(all.size(), 0);
  for (size_t i = 0; i < all.size(); ++i) {
    pl.ns[i].n = all[i];
    pl.ns[i].h = all[i]->out;
    all[i]->plan_idx = (int)i;
  }
  for (size_t i = 0; i < all.size(); ++i) {
    PN& pn = pl.ns[i];
    Node* n = pn.n;
    pn.prod.resize(n->in.size());
    bool all_const = true;
    for (size_t k = 0; k < n->in.size(); ++k) {
      const int q = pn_of(pl, n->in[k]);
      pn.prod[k] = q;
      if (q >= 0) {
        add_unique(pl.ns[q].cons, (int)i);
        if (!pl.ns[q].is_const) all_const = false;
      } else {
        all_const = false;
      }
    }
    // constants: FILL, and scale / smooth closures / sums over constants (the seed of gradTOp and its negation)
    const int op = n->d.op;
    if (op == N_FILL) {
      pn.is_const = true;
      pn.cval = n->d.alpha;
    } else if (all_const && !n->in.empty() && n->in.size() <= 8 && (op == N_SCALE || op == N_SUM || op == N_LIFT)) {
      double x[8] = {0};
      for (size_t k = 0; k < n->in.size(); ++k) x[k] = pl.ns[pn.prod[k]].cval;
      bool same_shapes = true;
      for (to_tensor in : n->in) same_shapes = same_shapes && same_shape(in, pn.h);
      if (same_shapes) {
        pn.is_const = true;
        if (op == N_SCALE) pn.cval = n->d.alpha * x[0];
        else if (op == N_SUM) {
          pn.cval = 0.0;
          for (size_t k = 0; k < n->in.size(); ++k) pn.cval += pl.ns[pn.prod[k]].cval;
        } else {
          pn.cval = expr_eval(*n->d.f, x);
        }
      }
    }
  }
}

// ancestor bitsets (planning only: a plan that comes out of the cache does not need them)
void compute_ancestors(Plan& pl) {
  const size_t N = pl.ns.size();
  pl.words = (int)((N + 63) / 64);
  pl.anc.assign(N, std::vector<uint64_t>((size_t)pl.words, 0));
  for (size_t i = 0; i < N; ++i)
    for (int q : pl.ns[i].prod)
      if (q >= 0) {
        for (int w = 0; w < pl.words; ++w) pl.anc[i][w] |= pl.anc[q][w];
        pl.anc[i][q >> 6] |= 1ull << (q & 63);
      }
}

// ---- tiny host tensors: the planner evaluates candidate loss heads on them -------------------------------------------
struct HT {
  int rank = 0;
  int64_t dims[TO_MAX_RANK] = {0};
  int64_t batch = 0;
  std::vector<double> v;
  int64_t numel() const {
    int64_t n = 1;
    for (int i = 0; i < rank; ++i) n *= dims[i];
    return n;
  }
  double at(int64_t b, int64_t e) const { return v[(size_t)((batch > 0 ? b : 0) * numel() + e)]; }
};
static HT ht_like(to_tensor t, int64_t B) {
  HT h;
  h.rank = t->rank;
  for (int i = 0; i < t->rank; ++i) h.dims[i] = t->dims[i];
  h.batch = t->batch > 0 ? B : 0;
  h.v.assign((size_t)(h.numel() * (h.batch > 0 ? h.batch : 1)), 0.0);
  return h;
}

// would adding a node with these inputs to a group with these members close a cycle through other groups?
// (an outside input that descends from a member would have to run both after and before the group)
static bool inputs_clear_of(const Plan& pl, const std::vector<int>& members, int cand) {
  for (int q : pl.ns[cand].prod) {
    if (q < 0) continue;
    if (std::find(members.begin(), members.end(), q) != members.end()) continue;
    for (int m : members)
      if (m == q || pl.is_anc(m, q)) return false;
  }
  return true;
}

static bool sole_consumer(const Plan& pl, int i) {
  return pl.ns[i].cons.size() == 1 && !pl.ns[i].demanded && !pl.ns[i].copy_dst;
}

// ---- loss-head recognition ---------------------------------------------------------------------------------------------
static bool ht_eval_node(const Plan& pl, int i, const std::unordered_map<int, HT>& env, to_tensor target,
                         const HT& target_val, int64_t B, HT* out) {
  const PN& pn = pl.ns[i];
  const Node* n = pn.n;
  std::vector<HT> tmp;
  tmp.reserve(n->in.size());
  std::vector<const HT*> xs;
  for (size_t k = 0; k < n->in.size(); ++k) {
    const int q = pn.prod[k];
    if (q >= 0) {
      if (pl.ns[q].is_const) {
        HT c = ht_like(n->in[k], B);
        std::fill(c.v.begin(), c.v.end(), pl.ns[q].cval);
        tmp.push_back(std::move(c));
        xs.push_back(nullptr);  // fixed up below (tmp may reallocate)
        continue;
      }
      auto it = env.find(q);
      if (it == env.end()) return false;
      xs.push_back(&it->second);
    } else {
      if (!target || n->in[k]->ptr != target->ptr) return false;
      xs.push_back(&target_val);
    }
  }
  {
    size_t t = 0;
    for (size_t k = 0; k < xs.size(); ++k)
      if (!xs[k]) xs[k] = &tmp[t++];
  }
  HT r = ht_like(pn.h, B);
  const int64_t ne = r.numel(), nb = r.batch > 0 ? r.batch : 1;
  switch (n->d.op) {
    case N_LIFT: {
      double x[8];
      for (int64_t b = 0; b < nb; ++b)
        for (int64_t e = 0; e < ne; ++e) {
          for (size_t k = 0; k < xs.size(); ++k) x[k] = xs[k]->at(b, e);
          r.v[(size_t)(b * ne + e)] = expr_eval(*n->d.f, x);
        }
      break;
    }
    case N_DACT:
      for (int64_t b = 0; b < nb; ++b)
        for (int64_t e = 0; e < ne; ++e) {
          const double d = xs[0]->at(b, e), h = xs[1]->at(b, e);
          r.v[(size_t)(b * ne + e)] = n->d.lm ? d * (1.0 - h * h) : d * h * (1.0 - h);
        }
      break;
    case N_SUM:
      for (int64_t b = 0; b < nb; ++b)
        for (int64_t e = 0; e < ne; ++e) {
          double a = 0.0;
          for (const HT* x : xs) a += x->at(b, e);
          r.v[(size_t)(b * ne + e)] = a;
        }
      break;
    case N_SCALE:
      for (int64_t b = 0; b < nb; ++b)
        for (int64_t e = 0; e < ne; ++e) r.v[(size_t)(b * ne + e)] = n->d.alpha * xs[0]->at(b, e);
      break;
    case N_SUM_ROWS: {
      const int64_t R = xs[0]->dims[0];
      for (int64_t b = 0; b < nb; ++b)
        for (int64_t e = 0; e < ne; ++e) {
          double a = 0.0;
          for (int64_t q = 0; q < R; ++q) a += xs[0]->at(b, q * ne + e);
          r.v[(size_t)(b * ne + e)] = a;
        }
      break;
    }
    case N_MAP_ROWS: {
      const int64_t J = xs[0]->numel();
      for (int64_t b = 0; b < nb; ++b)
        for (int64_t e = 0; e < ne; ++e) r.v[(size_t)(b * ne + e)] = xs[0]->at(b, J ? e % J : 0);
      break;
    }
    case N_GMUL: {
      if (n->d.reduce || n->d.lo > 1) return false;
      int64_t M = 1, K = 1, N = 1;
      for (int k = 0; k < n->d.lm; ++k) M *= xs[0]->dims[k];
      for (int k = 0; k < n->d.lo; ++k) K *= xs[0]->dims[n->d.lm + k];
      for (int k = 0; k < n->d.ln; ++k) N *= xs[1]->dims[n->d.lo + k];
      for (int64_t b = 0; b < nb; ++b)
        for (int64_t m = 0; m < M; ++m)
          for (int64_t c = 0; c < N; ++c) {
            double a = 0.0;
            for (int64_t k = 0; k < K; ++k) a += xs[0]->at(b, m * K + k) * xs[1]->at(b, k * N + c);
            r.v[(size_t)(b * ne + m * N + c)] = a;
          }
      break;
    }
    default: return false;
  }
  *out = std::move(r);
  return true;
}

static bool ht_close(double a, double b) {
  if (!std::isfinite(a) || !std::isfinite(b)) return false;
  return std::fabs(a - b) <= 1e-9 * (1.0 + std::fabs(a) + std::fabs(b));
}

// The row-local subgraph hanging off `root` ([B x N], the result of gmul + bias): if the only thing the rest of
// the graph needs from it is dz [B x N] (and possibly a per-row loss) and dz(z, t) is one of the two closed forms
// the small-GEMM kernel's loss head computes, fill in the group.  Probabilistic identity testing, as for
// closures (expr.cpp): only smooth programs are considered, so agreement on random rows means identity.
// The recognition is an identity TEST (three scales of logits, three rows each, 1e-9), not a proof: a false positive would be
// a silently wrong gradient.  A host that would rather pay the launches can turn it off: TOPS_LOSS_HEAD_MATCH=0 for the
// process, to_set_loss_head_match for what is planned from now on (the state is part of a plan's signature, so a cached plan
// made under the other setting is not reused).  Off, the same subgraph runs as a row program or op by op.
static int g_loss_head_match = -1;
bool loss_head_match_on() {
  if (g_loss_head_match < 0) {
    const char* e = getenv("TOPS_LOSS_HEAD_MATCH");
    g_loss_head_match = !(e && e[0] == '0');
  }
  return g_loss_head_match != 0;
}
int lazy_set_loss_head_match(int on) {
  const int prev = loss_head_match_on() ? 1 : 0;
  g_loss_head_match = on ? 1 : 0;
  return prev;
}

static bool match_loss_head(Plan& pl, Gr& g, int root) {
  if (!loss_head_match_on()) return false;
  to_tensor rh = pl.ns[root].h;
  // (batched: one row per sample; unbatched: the single row of a per-sample step)
  if (rh->rank != 1 || rh->dims[0] < 1 || rh->dims[0] > 16) return false;
  const int64_t N = rh->dims[0], Bfull = rh->batch;
  std::vector<int> S{root}, K;  // members, constants they use
  std::vector<char> inS(pl.ns.size(), 0);
  inS[root] = 1;
  to_tensor target = nullptr;
  Ref target_ref;
  for (size_t i = (size_t)root + 1; i < pl.ns.size(); ++i) {
    PN& pn = pl.ns[i];
    if (pl.d.group[i] >= 0 || pn.is_const) continue;
    const Node* n = pn.n;
    const int op = n->d.op;
    if (!(op == N_LIFT || op == N_DACT || op == N_SUM || op == N_SCALE || op == N_SUM_ROWS || op == N_MAP_ROWS ||
          (op == N_GMUL && !n->d.reduce && n->d.lo <= 1)))
      continue;
    if (op == N_LIFT && !expr_is_smooth(*n->d.f)) continue;
    // the result: one row (or one number) per sample
    if (pn.h->batch != Bfull || pn.h->rank > 1 || (pn.h->rank == 1 && pn.h->dims[0] != N)) continue;
    bool any_in = false, ok = true;  // any_in: reads a member or the target rows
    to_tensor tgt = target;
    Ref tgt_ref = target_ref;
    for (size_t k = 0; k < n->in.size() && ok; ++k) {
      to_tensor x = n->in[k];
      const int q = pn.prod[k];
      if (q >= 0) {
        if (inS[q]) {
          any_in = true;
          ok = same_value_layout(x, pl.ns[q].h);
        } else if (pl.ns[q].is_const) {
          ok = x->rank <= 1;
        } else {
          ok = false;
        }
      } else {
        // an existing value: the target rows (one operand only)
        ok = x->batch == Bfull && x->rank == 1 && x->dims[0] == N && x->contiguous() && x->dtype == rh->dtype &&
             (!tgt || tgt->ptr == x->ptr);
        if (ok) {
          if (!tgt) tgt_ref = Ref{(int)i, (int)k};
          tgt = x;
          any_in = true;
        }
      }
    }
    if (!ok || !any_in) continue;
    target = tgt;
    target_ref = tgt_ref;
    inS[i] = 1;
    S.push_back((int)i);
  }
  if (S.size() < 2 || !target) return false;
  // what the rest of the graph reads from S
  int dz = -1, loss = -1;
  for (int i : S) {
    const PN& pn = pl.ns[i];
    bool outside = pn.demanded || pn.copy_dst;
    for (int c : pn.cons)
      if (!inS[c]) outside = true;
    if (!outside) continue;
    if (pn.h->rank == 1 && dz < 0 && i != root) dz = i;
    else if (pn.h->rank == 0 && loss < 0) loss = i;
    else return false;
  }
  if (dz < 0) return false;
  // Evaluate on random rows at three scales -- logits in (-2, 2), (-6, 6) and (-0.1, 0.1), three rows each (one each
  // for the single row of an unbatched step).  Members are compositions of +, *, /, exp, log, tanh ... (expr_is_smooth:
  // nothing piecewise), i.e. real-analytic in (z, t) on the connected domain where they are defined, and so are the
  // closed forms: two analytic maps that agree on a set with an accumulation point are the same map, and a map that is
  // NOT the closed form differs from it everywhere except on a set of measure zero -- points in general position at
  // three scales do not lie on it.  What can slip through is a program within 1e-9 relative of the closed form at every
  // scale, whose gradient is then wrong by that much.
  const int64_t B = 3;
  struct Lcg {
    uint64_t s = 0x7e500002ull;
    double next() {
      s = s * 6364136223846793005ull + 1442695040888963407ull;
      return ((s >> 11) + 0.5) * (1.0 / 9007199254740992.0);
    }
  } rng;
  int kind = 0;
  const double half_width[3] = {2.0, 6.0, 0.1};
  for (int trial = 0; trial < 3; ++trial) {
    HT z = ht_like(rh, B), t = ht_like(target, B);
    for (double& x : z.v) x = half_width[trial] * (2.0 * rng.next() - 1.0);
    for (double& x : t.v) x = 0.05 + rng.next();
    std::unordered_map<int, HT> env;
    env[root] = z;
    for (size_t k = 1; k < S.size(); ++k) {
      HT r;
      if (!ht_eval_node(pl, S[k], env, target, t, B, &r)) return false;
      env[S[k]] = std::move(r);
    }
    const HT& got = env[dz];
    int kind_here = 0;
    for (int cand = 1; cand <= 2 && !kind_here; ++cand) {
      bool ok = true;
      for (int64_t b = 0; b < B && ok; ++b) {
        double se = 0.0, sy = 0.0, mx = -1e300, lossv = 0.0;
        for (int64_t j = 0; j < N; ++j) mx = std::max(mx, z.at(b, j));
        for (int64_t j = 0; j < N; ++j) {
          se += std::exp(z.at(b, j) - mx);
          sy += t.at(b, j);
        }
        for (int64_t j = 0; j < N && ok; ++j) {
          double want;
          if (cand == 1) {
            const double pr = std::exp(z.at(b, j) - mx) / se;
            want = pr * sy - t.at(b, j);
            lossv += -t.at(b, j) * std::log(pr);
          } else {
            const double s = 1.0 / (1.0 + std::exp(-z.at(b, j))), e = t.at(b, j) - s;
            want = -2.0 * e * s * (1.0 - s);
            lossv += e * e;
          }
          ok = ht_close(got.at(b, j), want);
        }
        if (ok && loss >= 0) ok = ht_close(env[loss].at(b, 0), lossv);
      }
      if (ok) kind_here = cand;
    }
    if (!kind_here || (trial > 0 && kind_here != kind)) return false;
    kind = kind_here;
  }
  if (!kind) return false;
  // constants used only inside S ride along (never stored when the head is fused)
  for (int i : S)
    for (int q : pl.ns[i].prod)
      if (q >= 0 && pl.ns[q].is_const && pl.d.group[q] < 0 && !pl.ns[q].demanded && !pl.ns[q].copy_dst) {
        bool all_in = true;
        for (int c : pl.ns[q].cons)
          if (!inS[c]) all_in = false;
        if (all_in) add_unique(K, q);
      }
  // (constants of constants: one more level covers `negate` of the seed)
  for (size_t k = 0; k < K.size(); ++k)
    for (int q : pl.ns[K[k]].prod)
      if (q >= 0 && pl.ns[q].is_const && pl.d.group[q] < 0 && !pl.ns[q].demanded && !pl.ns[q].copy_dst) {
        bool all_in = true;
        for (int c : pl.ns[q].cons)
          if (!inS[c] && std::find(K.begin(), K.end(), c) == K.end()) all_in = false;
        if (all_in) add_unique(K, q);
      }
  for (size_t k = 1; k < S.size(); ++k) g.mem.push_back(S[k]);
  for (int q : K) g.mem.push_back(q);
  g.loss_kind = kind;
  g.target = target_ref;
  g.loss_node = loss;
  g.out = dz;
  return true;
}

// ---- grouping -----------------------------------------------------------------------------------------------------------
// `d * logistic'(z)` (EW_MUL_DLOGISTIC on [d, z]) where h = logistic(z) is part of the graph: consume h instead.
// The forward value is always there (the next layer needed it), and z = gmul + bias then has one consumer less --
// which is what lets it stay inside the GEMM launch.
static void rewrite_dlogistic(Plan& pl) {
  for (size_t i = 0; i < pl.ns.size(); ++i) {
    Node* n = pl.ns[i].n;
    if (n->d.op != N_LIFT || (n->d.f->kind != EW_MUL_DLOGISTIC && n->d.f->kind != EW_MUL_DTANH) || n->in.size() != 2) continue;
    const int fwd_kind = n->d.f->kind == EW_MUL_DTANH ? EW_TANH : EW_LOGISTIC;
    const int zq = pl.ns[i].prod[1];
    if (zq < 0) continue;
    to_tensor z = n->in[1];
    if (!same_value_layout(z, pl.ns[zq].h)) continue;
    for (int c : pl.ns[zq].cons) {
      Node* m = pl.ns[c].n;
      if ((size_t)c == i || m->d.op != N_LIFT || m->d.f->kind != fwd_kind || !same_value_layout(m->in[0], pl.ns[zq].h))
        continue;
      if (!full_like(pl.ns[c].h, pl.ns[i].h)) continue;
      apply_dlogistic(pl, (int)i, c);  // rewrite in place: the node now reads h
      pl.d.dlogistic.emplace_back((int)i, c);
      break;
    }
  }
}

// node i of the plan reads h = logistic(z), the value of node c, instead of z: `d * logistic'(z)` becomes d * h (1 - h)
void apply_dlogistic(Plan& pl, int i, int c) {
  Node* n = pl.ns[i].n;
  to_tensor z = n->in[1], h = pl.ns[c].h;
  const int zq = pl.ns[i].prod[1];
  retain_int(h);
  n->in[1] = h;
  const int tanh_form = n->d.f->kind == EW_MUL_DTANH ? 1 : 0;
  expr_release(n->d.f);
  n->d.f = nullptr;
  n->d.op = N_DACT;
  n->d.lm = tanh_form;
  pl.ns[i].prod[1] = c;
  if (zq >= 0 && pl.ns[i].prod[0] != zq) {  // (`d * logistic'(d)`: the node still reads z as its first input)
    auto& zc = pl.ns[zq].cons;
    zc.erase(std::remove(zc.begin(), zc.end(), i), zc.end());
  }
  add_unique(pl.ns[c].cons, i);
  release_int(z);
}

static void form_gemm_group(Plan& pl, int a) {
  PN& an = pl.ns[a];
  Node* n = an.n;
  GmulPlan gp;
  dry_plan(n, gp);
  Gr g;
  g.gemm = true;
  g.anchor = a;
  g.mem.push_back(a);
  int cur = a;
  const bool plain_layout = gp.exact && !gp.zero && gp.p.batch == 1 && !gp.p.reduce_batch;
  // C as the kernels see it: [p.M x p.N] row-major in the result's own storage
  const GemmProblem& p = gp.p;
  int stage = 0;  // 0 linear part, 1 bias added, 2 activation applied, 3 dact applied
  // the loss head (and its tail) behind a bare gmul + bias whose rows fit one 16-lane group
  bool head_done = false;
  auto try_loss_head = [&]() {
    if (head_done || !(plain_layout && gp.rows_are_samples && stage <= 1 && !g.cin && g.beta == 0.0 && p.N <= 16)) return false;
    GemmProblem q = p;
    q.alpha = g.alpha;
    if (!gemm_small_fuses_loss(q)) return false;
    Gr trial = g;
    if (!match_loss_head(pl, trial, cur)) return false;
    g = trial;
    head_done = true;
    // tail: T = (gmul W^T dz) * h (1 - h), one 16-row block of T per workgroup of the same launch
    const int dz = g.out;
    for (int c : pl.ns[dz].cons) {
      PN& cn = pl.ns[c];
      Node* m = cn.n;
      if (pl.d.group[c] >= 0 || m->d.op != N_GMUL || m->d.reduce || !sole_consumer(pl, c)) continue;
      if (cn.prod[1] != dz || !same_value_layout(m->in[1], pl.ns[dz].h) || cn.prod[0] >= 0) continue;
      const int tq = cn.cons[0];
      PN& tn = pl.ns[tq];
      if (pl.d.group[tq] >= 0 || tn.n->d.op != N_DACT || tn.n->d.lm != 0 || tn.prod[0] != c || !same_value_layout(tn.n->in[0], cn.h)) continue;
      if (!full_like(tn.n->in[1], tn.h) || tn.h->rank != 1 || tn.h->batch != pl.ns[dz].h->batch) continue;
      GmulPlan tp;
      dry_plan(m, tp);
      const int64_t tail_n = tn.h->dims[0];
      if (!tp.exact || tp.zero || !tp.rows_are_samples || tp.p.batch != 1 || tp.p.K != p.N || tp.p.N != tail_n ||
          tp.p.b_sk != tail_n || tp.p.b_sn != 1 || tp.p.a_sk != 1 || tp.p.a_sm != p.N)
        continue;
      if (!gemm_small_fuses_tail(q, tail_n)) continue;
      std::vector<int> with = g.mem;
      with.push_back(c);
      if (!inputs_clear_of(pl, with, tq) || !inputs_clear_of(pl, g.mem, c)) continue;
      g.mem.push_back(c);
      g.mem.push_back(tq);
      g.tail = tq;
      g.tail_w = Ref{c, 0};
      g.tail_h = Ref{tq, 1};
      break;
    }
    return true;
  };
  while (plain_layout && sole_consumer(pl, cur) && !head_done) {
    const int c = pl.ns[cur].cons[0];
    PN& cn = pl.ns[c];
    if (pl.d.group[c] >= 0) break;
    Node* m = cn.n;
    // which input is the running value?
    int pos = -1;
    for (size_t k = 0; k < m->in.size(); ++k)
      if (cn.prod[k] == cur && same_value_layout(m->in[k], pl.ns[cur].h)) pos = (int)k;
    if (pos < 0) break;
    int uses = 0;
    for (int q : cn.prod) uses += q == cur;
    if (uses != 1) break;
    if (!full_like(cn.h, pl.ns[cur].h)) break;
    if (!inputs_clear_of(pl, g.mem, c)) break;
    bool took = false;
    const int op = m->d.op;
    if (op == N_SCALE && stage == 0) {
      g.alpha *= m->d.alpha;
      g.beta *= m->d.alpha;
      took = true;
    } else if ((op == N_SUM && m->in.size() == 2) ||
               (op == N_LIFT && m->d.f->kind == EW_AFFINE && m->in.size() == 2 && m->d.f->c0_d == 0.0)) {
      to_tensor other = m->in[1 - pos];
      double ca = 1.0, co = 1.0;  // coefficients of the running value / of the other operand
      if (op == N_LIFT) {
        ca = m->d.f->coef_d[pos];
        co = m->d.f->coef_d[1 - pos];
      }
      const bool bias_like = gp.rows_are_samples && other->batch == 0 && other->rank == 1 && cn.h->rank == 1 &&
                             other->dims[0] == p.N && other->contiguous() && co == 1.0;
      if (stage == 0 && bias_like && ca != 0.0) {
        g.alpha *= ca;
        g.beta *= ca;
        g.bias = Ref{c, 1 - pos};
        stage = 1;
        took = true;
      } else if (stage == 0 && !g.cin && full_like(other, cn.h) && ca != 0.0) {
        g.alpha *= ca;
        g.cin = Ref{c, 1 - pos};
        g.beta = co;
        took = true;
      }
    } else if (op == N_LIFT && m->d.f->kind == EW_AFFINE && m->in.size() == 1 && m->d.f->c0_d == 0.0 && stage == 0) {
      g.alpha *= m->d.f->coef_d[0];
      g.beta *= m->d.f->coef_d[0];
      took = true;
    } else if (op == N_LIFT && m->d.f->kind == EW_LOGISTIC && stage <= 1) {
      // (an output layer: logistic >>> squaredError's backward reads this value -- the loss head takes all of it)
      if (try_loss_head()) break;
      g.act = 1;
      stage = 2;
      took = true;
    } else if (op == N_LIFT && m->d.f->kind == EW_TANH && stage <= 1) {
      g.act = 2;
      stage = 2;
      took = true;
    } else if (op == N_DACT && pos == 0 && stage <= 1 && full_like(m->in[1], cn.h)) {
      g.dact = Ref{c, 1};
      g.dact_kind = m->d.lm;
      stage = 3;
      took = true;
    }
    if (!took) break;
    g.mem.push_back(c);
    cur = c;
  }
  if (!head_done) {
    g.out = cur;
    try_loss_head();
  }
  // the weight-gradient form dW = sum_b dz_b (x) a_b = dZ^T A next to db = sum_b dz_b: the row sums of the
  // A operand come out of the same launch
  const bool outer1 = !n->d.reduce && n->d.lm == 1 && n->d.lo == 0 && n->d.ln == 1 && n->in[0]->batch == 0 &&
                      n->in[1]->batch == 0;  // dz (x) a of a per-sample step
  if (plain_layout && (n->d.reduce || outer1) && !g.loss_kind && g.act == 0 && !g.dact && !g.bias) {
    g.wgrad_like = true;
    to_tensor dzh = n->in[0];
    // The row sums ride along in the small-GEMM kernel only.  A weight gradient beyond its range (a 4096 -> 4096 layer: dW is
    // 4096 x B x 4096) keeps its own epilogue -- W - r dW as alpha A B + beta Cin, produced in place -- and leaves the bias
    // gradient to a launch of its own; with the sibling attached the whole group used to fall apart into GEMM, update, sum,
    // update and a copy of W (tools/step_scan.py: 4096-4096-10 at 32 rows 193 us a step, torch 125).
    const bool rs_rides = gemm_small_route(p);
    if (rs_rides && outer1 && an.prod[0] >= 0 && p.K == 1) {
      // the bias update of the same layer reads dz itself (no batch to sum over): b - r*dz rides along as the
      // "row sums" of the one-column A operand
      const int dq = an.prod[0];
      for (int c : pl.ns[dq].cons) {
        PN& cn = pl.ns[c];
        Node* m = cn.n;
        if (g.rs >= 0 || pl.d.group[c] >= 0 || c == a || m->d.op != N_LIFT || m->d.f->kind != EW_AFFINE || m->in.size() != 2 ||
            m->d.f->c0_d != 0.0)
          continue;
        int pos = -1;
        for (int k = 0; k < 2; ++k)
          if (cn.prod[k] == dq && same_value_layout(m->in[k], pl.ns[dq].h) && same_value_layout(dzh, pl.ns[dq].h)) pos = k;
        if (pos < 0 || cn.prod[1 - pos] == dq || m->d.f->coef_d[1 - pos] != 1.0 || !full_like(m->in[1 - pos], cn.h) ||
            !full_like(cn.h, pl.ns[dq].h) || m->d.f->coef_d[pos] != g.alpha)
          continue;
        if (!inputs_clear_of(pl, g.mem, c)) continue;
        bool indep = true;
        for (int mm : g.mem)
          if (pl.is_anc(mm, c) || pl.is_anc(c, mm)) indep = false;
        if (!indep) continue;
        g.mem.push_back(c);
        g.rs = c;
        g.rs_in = Ref{c, 1 - pos};
        g.rs_alpha = m->d.f->coef_d[pos];
      }
    }
    if (rs_rides && dzh->batch > 0 && dzh->rank == 1 && n->d.lm == 1 && n->d.lo == 0 && (p.a_sm == 1 || p.M == 1) &&
        (p.a_sk == p.M || p.K == 1) && p.K == dzh->batch) {
      const int dq = an.prod[0];
      // siblings: batch_sum of the same value
      auto try_sibling = [&](int r) {
        PN& rn = pl.ns[r];
        if (pl.d.group[r] >= 0 || rn.n->d.op != N_BATCH_SUM || r == a) return false;
        to_tensor x = rn.n->in[0];
        if (!(x == dzh || (x->ptr && x->ptr == dzh->ptr && full_like(x, dzh)) ||
              (dq >= 0 && rn.prod[0] == dq && same_value_layout(x, pl.ns[dq].h) && same_value_layout(dzh, pl.ns[dq].h))))
          return false;
        std::vector<int> with = g.mem;
        if (!inputs_clear_of(pl, with, r)) return false;
        for (int mm : g.mem)
          if (pl.is_anc(mm, r) || pl.is_anc(r, mm)) return false;
        g.mem.push_back(r);
        g.rs = r;
        // p_b - rate * db: the bias update in the same epilogue
        if (sole_consumer(pl, r)) {
          const int c = rn.cons[0];
          PN& cn = pl.ns[c];
          Node* m = cn.n;
          if (pl.d.group[c] < 0 && m->d.op == N_LIFT && m->d.f->kind == EW_AFFINE && m->in.size() == 2 && m->d.f->c0_d == 0.0) {
            int pos = -1;
            for (int k = 0; k < 2; ++k)
              if (cn.prod[k] == r && same_value_layout(m->in[k], rn.h)) pos = k;
            if (pos >= 0 && cn.prod[1 - pos] != r && m->d.f->coef_d[1 - pos] == 1.0 && full_like(m->in[1 - pos], rn.h) &&
                full_like(cn.h, rn.h) && inputs_clear_of(pl, g.mem, c)) {
              g.mem.push_back(c);
              g.rs = c;
              g.rs_in = Ref{c, 1 - pos};
              g.rs_alpha = m->d.f->coef_d[pos];
            }
          }
        }
        return true;
      };
      bool found = false;
      if (dq >= 0) {
        for (int r : pl.ns[dq].cons)
          if (!found && try_sibling(r)) found = true;
      } else {
        for (size_t r = 0; r < pl.ns.size() && !found; ++r)
          if (try_sibling((int)r)) found = true;
      }
    }
  }
  std::sort(g.mem.begin(), g.mem.end());
  const int gi = (int)pl.d.gs.size();
  for (int m : g.mem) pl.d.group[m] = gi;
  pl.d.gs.push_back(std::move(g));
}

static bool path_between(const Plan& pl, const Gr& from, const Gr& to) {  // does `to` depend on `from`?
  for (int a : from.mem)
    for (int b : to.mem)
      if (a == b || pl.is_anc(a, b)) return true;
  return false;
}

// ---- row programs: what hangs off a GEMM group's output and only ever touches one row at a time -------------------------
// (loss heads wider than the 16 lanes of the small-GEMM epilogue, heads the library has no closed form for: softmax >>>
//  scale >>> squaredError, an auto-encoder's squaredError over the whole input width ...)
static bool form_row_program_impl(Plan& pl, int root, bool allow_peers);
static void form_row_program(Plan& pl, int root) {
  // operands produced by OTHER launches of the same plan (the second GEMM of `W x + W' s + b`, Recurrent.hs:108-118) may
  // be read like existing tensors -- unless that closes a cycle through the program's own outputs; then without them
  if (!form_row_program_impl(pl, root, true)) form_row_program_impl(pl, root, false);
}
// true: done (a group was formed, or there is nothing to form); false: try again without peers
static bool form_row_program_impl(Plan& pl, int root, bool allow_peers) {
  to_tensor rh = pl.ns[root].h;
  if (rh->rank != 1 || rh->dims[0] < 1 || rh->dims[0] > 1024) return true;
  const int64_t N = rh->dims[0], Bfull = rh->batch;
  std::vector<to_tensor> ext;
  std::vector<Ref> ext_ref;
  std::vector<int> ext_q;  // producing plan node of a peer operand, -1 for an existing tensor
  std::vector<char> inT(pl.ns.size(), 0), inS(pl.ns.size(), 0);
  const char* inT_ptr = inT.data();
  // a peer: the stored output of a GEMM group that has already been formed
  auto peer_ok = [&](int q, to_tensor x) {
    if (!allow_peers || pl.d.group[q] < 0) return false;
    const Gr& pg = pl.d.gs[pl.d.group[q]];
    if (!(pg.gemm && (pg.out == q || pg.tail == q) && same_value_layout(x, pl.ns[q].h) && (x->batch == Bfull || x->batch == 0)))
      return false;
    // a peer that itself needs something this program computes would have to run both before and after it
    for (size_t m = (size_t)root + 1; m < (size_t)q; ++m)
      if (inT_ptr[m] && pl.is_anc((int)m, q)) return false;
    return true;
  };
  auto row_shaped = [&](to_tensor t) { return t->rank == 0 || (t->rank == 1 && t->dims[0] == N); };
  auto same_ext = [](to_tensor e, to_tensor x) { return e == x || (e->ptr && e->ptr == x->ptr && e->batch == x->batch && e->rank == x->rank); };
  // pass 1: T = row-local ops whose operands are the root, other members of T, constants or existing row-shaped tensors
  inT[root] = 1;
  for (size_t i = (size_t)root + 1; i < pl.ns.size(); ++i) {
    PN& pn = pl.ns[i];
    if (pl.d.group[i] >= 0 || pn.is_const || pn.copy_dst) continue;
    const Node* n = pn.n;
    const int op = n->d.op;
    if (!(op == N_LIFT || op == N_DACT || op == N_SUM || op == N_SCALE || op == N_SUM_ROWS || op == N_MAP_ROWS ||
          (op == N_GMUL && !n->d.reduce && n->d.lo <= 1)))
      continue;
    if (pn.h->batch != Bfull || !row_shaped(pn.h) || pn.h->dtype != rh->dtype || n->in.size() > 8) continue;
    if (op == N_MAP_ROWS && n->d.len_n != 1) continue;
    if (op == N_GMUL && !((n->d.lo == 1 && n->in[0]->rank == 1 && n->in[1]->rank == 1) ||
                          (n->d.lo == 0 && n->in[0]->rank + n->in[1]->rank <= 1)))
      continue;
    bool ok = true;
    for (size_t k = 0; k < n->in.size() && ok; ++k) {
      to_tensor x = n->in[k];
      const int q = pn.prod[k];
      if (!row_shaped(x) || x->dtype != rh->dtype) ok = false;
      else if (q >= 0) ok = inT[q] ? same_value_layout(x, pl.ns[q].h) : (pl.ns[q].is_const || peer_ok(q, x));
      else ok = x->ptr && x->contiguous() && (x->batch == Bfull || x->batch == 0);  // per row, or shared by all rows
    }
    if (ok) inT[i] = 1;
  }
  // pass 2: what the root reaches inside T; pass 3: plus what those need from T (the target's side of a loss:
  // `-y * seed` depends on no member, the cotangent that consumes it does)
  inS[root] = 1;
  for (size_t i = (size_t)root + 1; i < pl.ns.size(); ++i)
    if (inT[i])
      for (int q : pl.ns[i].prod)
        if (q >= 0 && inS[q]) inS[i] = 1;
  for (size_t i = pl.ns.size(); i-- > (size_t)root + 1;)
    if (inS[i])
      for (int q : pl.ns[i].prod)
        if (q >= 0 && inT[q]) inS[q] = 1;
  std::vector<int> S{root};
  for (size_t i = (size_t)root + 1; i < pl.ns.size(); ++i) {
    if (!inS[i]) continue;
    S.push_back((int)i);
    const Node* n = pl.ns[i].n;
    for (size_t k = 0; k < n->in.size(); ++k) {
      const int q = pl.ns[i].prod[k];
      if (q >= 0 && (inS[q] || pl.ns[q].is_const)) continue;
      bool known = false;
      for (size_t e = 0; e < ext.size(); ++e) known = known || (q >= 0 ? ext_q[e] == q : (ext_q[e] < 0 && same_ext(ext[e], n->in[k])));
      if (!known) {
        ext.push_back(n->in[k]);
        ext_ref.push_back(Ref{(int)i, (int)k});
        ext_q.push_back(q);
      }
    }
  }
  if (ext.size() > 4) return !allow_peers;
  if (S.size() < 3) return true;  // (the root and a single op: that op is one launch already)
  // a peer that itself needs something this program produces would have to run both before and after it
  for (int q : ext_q)
    if (q >= 0)
      for (size_t k = 1; k < S.size(); ++k)
        if (pl.is_anc(S[k], q)) return false;
  // what the rest of the graph needs from it
  std::vector<int> outs;
  for (size_t k = 1; k < S.size(); ++k) {
    const PN& pn = pl.ns[S[k]];
    bool outside = pn.demanded;
    for (int c : pn.cons)
      if (!inS[c]) outside = true;
    if (outside) outs.push_back(S[k]);
  }
  if (outs.empty() || outs.size() > 4) return true;
  // the program: value ids 0 = root, 1.. = existing tensors, then the nodes (constants are re-stated as literals)
  auto rp = std::make_shared<RowProg>();
  rp->dtype = rh->dtype;
  rp->N = N;
  for (to_tensor e : ext) {
    rp->ext_vec.push_back(e->rank == 1);
    rp->ext_rowwise.push_back(e->batch > 0 || Bfull == 0);
  }
  std::unordered_map<int, int> id_of;  // plan node -> value id
  id_of[root] = 0;
  std::unordered_map<int, int> const_id;
  auto ext_id = [&](to_tensor x, int q) {
    for (size_t e = 0; e < ext.size(); ++e)
      if (q >= 0 ? ext_q[e] == q : (ext_q[e] < 0 && same_ext(ext[e], x))) return 1 + (int)e;
    return -1;
  };
  const int base = 1 + (int)ext.size();
  for (size_t k = 1; k < S.size(); ++k) {
    const PN& pn = pl.ns[S[k]];
    const Node* n = pn.n;
    std::vector<int> in;
    for (size_t j = 0; j < n->in.size(); ++j) {
      const int q = pn.prod[j];
      if (q >= 0 && inS[q]) in.push_back(id_of[q]);
      else if (q >= 0 && !pl.ns[q].is_const) in.push_back(ext_id(n->in[j], q));  // a peer's output
      else if (q >= 0) {  // a constant
        auto it = const_id.find(q);
        if (it == const_id.end()) {
          RowNode c;
          c.op = R_CONST;
          c.vec = pl.ns[q].h->rank == 1;
          c.alpha = pl.ns[q].cval;
          rp->nodes.push_back(c);
          it = const_id.emplace(q, base + (int)rp->nodes.size() - 1).first;
        }
        in.push_back(it->second);
      } else {
        in.push_back(ext_id(n->in[j], -1));
      }
    }
    RowNode r;
    r.vec = pn.h->rank == 1;
    r.in = in;
    switch (n->d.op) {
      case N_LIFT: r.op = R_LIFT; r.f = n->d.f; expr_retain(r.f); break;
      case N_DACT: r.op = R_DACT; r.alpha = n->d.lm; break;
      case N_SUM: r.op = R_SUM; break;
      case N_SCALE: r.op = R_SCALE; r.alpha = n->d.alpha; break;
      case N_SUM_ROWS: r.op = R_SUM_ROWS; break;
      case N_MAP_ROWS: r.op = R_MAP_ROWS; break;
      default: r.op = n->d.lo == 1 ? R_DOT : R_MUL; break;  // gmul: a dot product, or a product with a scalar
    }
    rp->nodes.push_back(r);
    id_of[S[k]] = base + (int)rp->nodes.size() - 1;
  }
  for (int o : outs) rp->outs.push_back(id_of[o]);
  Gr g;
  g.rowprog = rp;
  g.rp_root = root;
  g.rp_outs = outs;
  g.rp_ext = ext_ref;
  for (size_t k = 1; k < S.size(); ++k) g.mem.push_back(S[k]);
  // constants used only in here never get storage
  for (auto& kv : const_id) {
    const PN& cn = pl.ns[kv.first];
    bool all_in = pl.d.group[kv.first] < 0 && !cn.demanded && !cn.copy_dst;
    for (int c : cn.cons)
      if (!inS[c]) all_in = false;
    if (all_in) g.mem.push_back(kv.first);
  }
  std::sort(g.mem.begin(), g.mem.end());
  g.out = outs[0];
  const int gi = (int)pl.d.gs.size();
  for (int m : g.mem) pl.d.group[m] = gi;
  pl.d.gs.push_back(std::move(g));
  return true;
}

// dependencies: outputs of other groups read by members
void group_deps(Plan& pl) {
  for (size_t gi = 0; gi < pl.d.gs.size(); ++gi) {
    Gr& g = pl.d.gs[gi];
    for (int m : g.mem)
      for (int q : pl.ns[m].prod)
        if (q >= 0 && pl.d.group[q] != (int)gi) add_unique(g.deps, pl.d.group[q]);
  }
}

void plan_groups(Plan& pl) {
  static const int fuse = [] { const char* e = getenv("TOPS_LAZY_FUSE"); return e ? atoi(e) : 1; }();
  if (fuse && pl.ns.size() <= 8192) {
    rewrite_dlogistic(pl);
    // a contraction of two per-row vectors / scalars (a dot product, a product with a scalar: the small change of a loss
    // head) is no GEMM: it is left for the row programs below, and becomes a launch of its own only if none takes it
    auto row_local = [&](int i) {
      const Node* n = pl.ns[i].n;
      return !n->d.reduce && n->d.lo <= 1 && n->in[0]->rank <= 1 && n->in[1]->rank <= 1 && pl.ns[i].h->rank <= 1;
    };
    for (size_t i = 0; i < pl.ns.size(); ++i)
      if (pl.d.group[i] < 0 && pl.ns[i].n->d.op == N_GMUL && !row_local((int)i)) form_gemm_group(pl, (int)i);
    // what is left hanging off the output of a GEMM group, row by row
    const size_t n_gemm_groups = pl.d.gs.size();
    for (size_t gi = 0; gi < n_gemm_groups; ++gi)
      if (pl.d.gs[gi].gemm && !pl.d.gs[gi].loss_kind && pl.d.gs[gi].out >= 0) form_row_program(pl, pl.d.gs[gi].out);
    for (size_t i = 0; i < pl.ns.size(); ++i)
      if (pl.d.group[i] < 0 && pl.ns[i].n->d.op == N_GMUL) form_gemm_group(pl, (int)i);
  }
  for (size_t i = 0; i < pl.ns.size(); ++i)
    if (pl.d.group[i] < 0) {
      Gr g;
      g.mem.push_back((int)i);
      g.out = (int)i;
      pl.d.group[i] = (int)pl.d.gs.size();
      pl.d.gs.push_back(std::move(g));
    }
  group_deps(pl);
  if (!fuse) return;
  // one-sample steps: every weight gradient is an outer product (K = 1).  All mutually independent ones go out
  // as ONE launch (rank1_many_kernel), with their `p - r*g` and bias updates
  {
    std::vector<int> r1;
    for (size_t gi = 0; gi < pl.d.gs.size(); ++gi) {
      Gr& g = pl.d.gs[gi];
      if (!g.gemm || !g.wgrad_like || g.act || g.dact || g.bias || g.loss_kind || g.tail >= 0) continue;
      if (g.cin && g.beta != 1.0) continue;
      GmulPlan gp;
      dry_plan(pl.ns[g.anchor].n, gp);
      if (!gp.exact || gp.zero || gp.p.K != 1 || gp.p.batch != 1 || (gp.p.a_sm != 1 && gp.p.M != 1) ||
          (gp.p.b_sn != 1 && gp.p.N != 1))
        continue;
      bool indep = true;
      for (int o : r1) indep = indep && !path_between(pl, pl.d.gs[o], g) && !path_between(pl, g, pl.d.gs[o]);
      if (indep && (int)r1.size() < RANK1_MAX_LAYERS) r1.push_back((int)gi);
    }
    if (r1.size() >= 2) {
      std::vector<int> deps;
      for (int gi : r1)
        for (int d : pl.d.gs[gi].deps) add_unique(deps, d);
      for (int gi : r1) {
        pl.d.gs[gi].r1 = r1[0];
        pl.d.gs[gi].deps = deps;
        pl.d.gs[gi].wgrad_like = false;  // not a pair candidate any more
      }
      pl.d.gs[r1[0]].r1_members = r1;
    }
  }
  // two independent weight-gradient GEMMs go out as one launch when the pair kernel takes their shapes
  std::vector<int> wg;
  for (size_t gi = 0; gi < pl.d.gs.size(); ++gi)
    if (pl.d.gs[gi].gemm && pl.d.gs[gi].wgrad_like) wg.push_back((int)gi);
  for (size_t a = 0; a < wg.size(); ++a)
    for (size_t b = a + 1; b < wg.size(); ++b) {
      Gr &g1 = pl.d.gs[wg[a]], &g2 = pl.d.gs[wg[b]];
      if (g1.pair >= 0 || g2.pair >= 0) continue;
      if (path_between(pl, g1, g2) || path_between(pl, g2, g1)) continue;
      // a third group between them (g1 -> x -> g2) is impossible without a path g1 -> g2
      GmulPlan p1, p2;
      dry_plan(pl.ns[g1.anchor].n, p1);
      dry_plan(pl.ns[g2.anchor].n, p2);
      if (!p1.exact || !p2.exact || !gemm_small_route(p1.p) || !gemm_small_route(p2.p)) continue;
      g1.pair = wg[b];
      g2.pair = wg[a];
      for (int d : g2.deps) add_unique(g1.deps, d);
      g2.deps = g1.deps;
    }
}

// to_copy_into destinations: produce the source straight into the destination when the source is an output of a
// fused launch, nothing else needs it, and every other reader of the destination's memory in this flush can be
// ordered before the launch
void plan_forwarding(Plan& pl) {
  for (size_t i = 0; i < pl.ns.size(); ++i) {
    PN& pn = pl.ns[i];
    if (!pn.copy_dst || pn.demanded || !pn.cons.empty()) continue;
    const int gi = pl.d.group[i];
    Gr& g = pl.d.gs[gi];
    if (!g.gemm || !((int)i == g.out || (int)i == g.rs || (int)i == g.tail || (int)i == g.loss_node)) continue;
    to_tensor d = pn.copy_dst;
    bool ok = true;
    std::vector<int> first;  // groups that must run before this one
    for (size_t k = 0; k < pl.ns.size() && ok; ++k) {
      const PN& o = pl.ns[k];
      for (size_t j = 0; j < o.n->in.size() && ok; ++j) {
        to_tensor x = o.n->in[j];
        if (o.prod[j] >= 0 || !x->ptr || !overlaps(x, d)) continue;
        const int og = pl.d.group[k];
        if (og == gi) {
          // inside the launch only an element-for-element alias is safe: Cin (or the bias being updated)
          const bool alias = x->ptr == d->ptr && full_like(x, d) &&
                             (((int)i == g.out && operand(pl, g.cin) == x) || ((int)i == g.rs && operand(pl, g.rs_in) == x));
          if (!alias) ok = false;
        } else if (g.r1 >= 0 && pl.d.gs[og].r1 == g.r1) {
          ok = false;  // another layer of the same launch reads it (never the case for a network's own parameters)
        } else if (path_between(pl, g, pl.d.gs[og]) || (g.pair >= 0 && path_between(pl, pl.d.gs[g.pair], pl.d.gs[og]))) {
          ok = false;  // that reader needs this launch's result: it cannot come first
        } else {
          first.push_back(og);
        }
      }
    }
    if (!ok) continue;
    pl.d.fwd[i] = 1;
    for (int f : first) {
      if (g.r1 >= 0)
        for (int m : pl.d.gs[g.r1].r1_members)
          if (m != f) add_unique(pl.d.gs[m].deps, f);
      add_unique(g.deps, f);
      if (g.pair >= 0 && f != g.pair) add_unique(pl.d.gs[g.pair].deps, f);
    }
  }
}

bool topo_order(Plan& pl) {
  std::vector<int>& order = pl.d.order;
  const int G = (int)pl.d.gs.size();
  std::vector<int> state(G, 0);
  order.clear();
  // iterative DFS; a pair is one unit (deps were merged)
  for (int root = 0; root < G; ++root) {
    if (state[root]) continue;
    std::vector<std::pair<int, size_t>> st{{root, 0}};
    state[root] = 1;
    while (!st.empty()) {
      auto& [g, k] = st.back();
      if (k < pl.d.gs[g].deps.size()) {
        int d = pl.d.gs[g].deps[k++];
        if (pl.d.gs[g].pair == d) continue;
        if (state[d] == 1) return false;  // cycle
        if (state[d] == 0) {
          state[d] = 1;
          st.push_back({d, 0});
        }
      } else {
        state[g] = 2;
        order.push_back(g);
        st.pop_back();
      }
    }
  }
  return true;
}

// ---- TOPS_LAZY_DEBUG=1: the plan of every flush on stderr -----------------------------------------------------------------
bool debug_on() {
  static const int on = [] { const char* e = getenv("TOPS_LAZY_DEBUG"); return e ? atoi(e) : 0; }();
  return on != 0;
}
static const char* op_name(int op) {
  switch (op) {
    case N_GMUL: return "gmul";
    case N_LIFT: return "lift";
    case N_SUM: return "sum";
    case N_SCALE: return "scale";
    case N_SUM_ROWS: return "sumRows";
    case N_MAP_ROWS: return "mapRows";
    case N_BATCH_SUM: return "batchSum";
    case N_FILL: return "fill";
    case N_DACT: return "dact";
    case N_STACK: return "stack";
    default: return "?";
  }
}
void dump_plan(const Plan& pl) {
  std::fprintf(stderr, "[lazy] flush: %zu nodes, %zu groups\n", pl.ns.size(), pl.d.gs.size());
  for (size_t i = 0; i < pl.ns.size(); ++i) {
    const PN& pn = pl.ns[i];
    std::fprintf(stderr, "  n%-3zu g%-3d %-8s%s %s <-", i, pl.d.group[i], op_name(pn.n->d.op),
                 pn.n->d.op == N_LIFT ? (" k" + std::to_string(pn.n->d.f->kind)).c_str() : "", shape_str(pn.h).c_str());
    for (size_t k = 0; k < pn.prod.size(); ++k) {
      if (pn.prod[k] >= 0) std::fprintf(stderr, " n%d", pn.prod[k]);
      else std::fprintf(stderr, " %s", shape_str(pn.n->in[k]).c_str());
    }
    std::fprintf(stderr, "  refs %d/%d v%zu%s%s%s%s\n", (int)pn.h->refs.load(), pn.h->int_refs, pn.h->dviews.size(), pn.demanded ? "  DEMANDED" : "", pn.copy_dst ? "  ->dst" : "", pl.d.fwd[i] ? "(in place)" : "",
                 pn.is_const ? "  const" : "");
  }
  for (size_t gi = 0; gi < pl.d.gs.size(); ++gi) {
    const Gr& g = pl.d.gs[gi];
    if (g.rowprog) {
      std::fprintf(stderr, "  g%zu: row program off n%d, %zu ops, %zu existing tensors, outputs", gi, g.rp_root, g.rowprog->nodes.size(),
                   g.rp_ext.size());
      for (int o : g.rp_outs) std::fprintf(stderr, " n%d", o);
      std::fprintf(stderr, "\n");
      continue;
    }
    if (!g.gemm || g.mem.size() == 1) continue;
    std::fprintf(stderr, "  g%zu: gemm n%d out n%d alpha %g beta %g%s%s%s%s rs n%d loss %d tail n%d pair g%d deps", gi, g.anchor,
                 g.out, g.alpha, g.beta, g.cin ? " cin" : "", g.bias ? " bias" : "", g.act ? " act" : "", g.dact ? " dact" : "",
                 g.rs, g.loss_kind, g.tail, g.pair);
    for (int d : g.deps) std::fprintf(stderr, " g%d", d);
    std::fprintf(stderr, "\n");
  }
}

}  // namespace to
