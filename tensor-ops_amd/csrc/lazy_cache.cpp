// The plan cache of the recorded class-method stream (lazy.cpp).
// A training loop records the same graph every step.  Everything the planner's decisions depend on goes into a signature:
// the recorded ops with their static arguments and expression ids, the graph's wiring, the layout of every operand that
// is not simply "the contiguous result of another node" (views, existing tensors), which existing tensors are the same
// memory or overlap, and what is demanded or copied where.  A cached plan IS the planner's decision record (Decisions,
// lazy_plan.hpp: the groups, their order, the forwarding decisions, the node rewrites), stored as the planner left it and
// copied back as it is: it names every operand by position ("input k of node i"), so the copy binds to this step's handles
// with nothing to re-bind, and a flush that finds its signature executes from the same record as the flush that planned it.
// Nothing that depends on addresses (alignment-driven kernel variants, packing) is in it: Exec::build works that out per
// launch.
#include <cstring>
#include <unordered_map>

#include "lazy_plan.hpp"

namespace to {

struct CachedPlan {
  std::vector<uint64_t> sig;
  Decisions d;
  mutable uint64_t used = 0;         // when it was last found (eviction is least-recently-used)
};
static uint64_t g_plan_clock = 0;
static std::unordered_map<uint64_t, std::vector<std::unique_ptr<CachedPlan>>>& plan_cache() {
  static std::unordered_map<uint64_t, std::vector<std::unique_ptr<CachedPlan>>> m;
  return m;
}
static size_t g_plan_cache_entries = 0;
static int64_t g_plan_cache_hits = 0, g_plan_cache_misses = 0;
void lazy_cache_stats(int64_t* hits, int64_t* misses, int64_t* entries) {
  if (hits) *hits = g_plan_cache_hits;
  if (misses) *misses = g_plan_cache_misses;
  if (entries) *entries = (int64_t)g_plan_cache_entries;
}
void lazy_cache_clear() {
  plan_cache().clear();
  g_plan_cache_entries = 0;
}
static bool plan_cache_on() {
  static const int on = [] { const char* e = getenv("TOPS_PLAN_CACHE"); return e ? atoi(e) : 1; }();
  return on != 0;
}

static uint64_t dbits(double d) {
  uint64_t u;
  std::memcpy(&u, &d, 8);
  return u;
}

static void sig_layout(std::vector<uint64_t>& s, to_tensor t) {
  s.push_back(((uint64_t)t->rank << 32) | ((uint64_t)t->dtype << 16) | (t->batch > 0 ? 1u : 0u));
  s.push_back((uint64_t)t->batch);
  s.push_back((uint64_t)t->bstride);
  for (int i = 0; i < t->rank; ++i) {
    s.push_back((uint64_t)t->dims[i]);
    s.push_back((uint64_t)t->strides[i]);
  }
}

static void plan_signature(const Plan& pl, std::vector<uint64_t>& s) {
  s.clear();
  s.reserve(pl.ns.size() * 24);
  std::vector<to_tensor> ext;  // existing tensors read by the plan, and the copy destinations
  // (found by hashing beyond a handful: the 513 operands of 512 sibling products were 131k pointer compares here and as many
  //  range tests below -- 0.65 ms of a flush whose two launches take 0.33)
  std::unordered_map<to_tensor, size_t> ext_ix;
  auto ext_slot = [&](to_tensor x) {
    if (ext.size() < 16) {
      for (size_t i = 0; i < ext.size(); ++i)
        if (ext[i] == x) return i;
    } else {
      if (ext_ix.empty())
        for (size_t i = 0; i < ext.size(); ++i) ext_ix.emplace(ext[i], i);
      auto it = ext_ix.find(x);
      if (it != ext_ix.end()) return it->second;
      ext_ix.emplace(x, ext.size());
    }
    ext.push_back(x);
    return ext.size() - 1;
  };
  s.push_back(pl.ns.size() | (loss_head_match_on() ? 0ull : 1ull << 62));
  for (size_t i = 0; i < pl.ns.size(); ++i) {
    const PN& pn = pl.ns[i];
    const Node* n = pn.n;
    s.push_back(((uint64_t)n->d.op << 48) | ((uint64_t)n->d.lm << 40) | ((uint64_t)n->d.lo << 32) | ((uint64_t)n->d.ln << 24) |
                ((uint64_t)n->d.reduce << 16) | (uint64_t)(n->d.len_n & 0xffff));
    s.push_back(dbits(n->d.alpha));
    // (the STRUCTURE of the closure, not the instance: a host that reifies its closures anew every step -- the Haskell
    //  shim's liftH does unless it caches them -- still repeats itself as far as a plan is concerned)
    s.push_back(n->d.f ? n->d.f->sid : 0);
    s.push_back(((uint64_t)n->in.size() << 8) | (pn.demanded ? 1u : 0u) | (pn.copy_dst ? 2u : 0u));
    sig_layout(s, pn.h);  // (a fresh result is contiguous: dims, batch and dtype are what matters)
    for (size_t k = 0; k < n->in.size(); ++k) {
      to_tensor x = n->in[k];
      const int q = pn.prod[k];
      if (q >= 0) {
        s.push_back(0x1000000000000000ull | (uint64_t)q);
        if (x == pl.ns[q].h) continue;
        s.push_back((uint64_t)x->view_off);  // a view of that node's value
        sig_layout(s, x);
      } else {
        s.push_back(0x2000000000000000ull | (uint64_t)ext_slot(x));
        sig_layout(s, x);
      }
    }
    if (pn.copy_dst) {
      s.push_back(0x3000000000000000ull | (uint64_t)ext_slot(pn.copy_dst));
      sig_layout(s, pn.copy_dst);
    }
  }
  // which existing tensors are the same memory / overlap (the target rows found twice, Cin aliasing a copy destination,
  // readers of memory that a forwarded result overwrites)
  s.push_back(0x4000000000000000ull | (uint64_t)ext.size());
  if (ext.size() < 16) {
    for (size_t a = 0; a < ext.size(); ++a)
      for (size_t b = a + 1; b < ext.size(); ++b) {
        const uint64_t rel = (ext[a]->ptr == ext[b]->ptr ? 1u : 0u) | (overlaps(ext[a], ext[b]) ? 2u : 0u);
        if (rel) s.push_back((a << 40) | (b << 8) | rel);
      }
  } else {
    // the same relation words in the same (a, b) order, found by a sweep over the address ranges instead of every pair
    struct R { const char *lo, *hi; size_t i; };
    std::vector<R> rs;
    rs.reserve(ext.size());
    for (size_t i = 0; i < ext.size(); ++i) {
      R r{nullptr, nullptr, i};
      if (ext[i]->ptr) mem_range(ext[i], &r.lo, &r.hi);
      rs.push_back(r);
    }
    std::sort(rs.begin(), rs.end(), [](const R& x, const R& y) { return x.lo < y.lo || (x.lo == y.lo && x.i < y.i); });
    std::vector<uint64_t> rel;
    for (size_t x = 0; x < rs.size(); ++x)
      for (size_t y = x + 1; y < rs.size(); ++y) {
        const bool same_ptr = rs[y].lo == rs[x].lo;                          // (null == null included, as in the pairwise form)
        const bool over = rs[x].lo && rs[y].lo < rs[x].hi && rs[x].lo < rs[y].hi;
        if (!same_ptr && !(rs[x].lo && rs[y].lo < rs[x].hi)) break;           // (sorted by lo: nothing further can touch x)
        const uint64_t w = (same_ptr ? 1u : 0u) | (over ? 2u : 0u);
        if (!w) continue;
        const size_t a = std::min(rs[x].i, rs[y].i), b = std::max(rs[x].i, rs[y].i);
        rel.push_back(((uint64_t)a << 40) | ((uint64_t)b << 8) | w);
      }
    std::sort(rel.begin(), rel.end());
    s.insert(s.end(), rel.begin(), rel.end());
  }
}

static uint64_t sig_hash(const std::vector<uint64_t>& s) {
  uint64_t h = 1469598103934665603ull;
  for (uint64_t v : s) {
    h ^= v;
    h *= 1099511628211ull;
    h ^= h >> 29;
  }
  return h;
}

static void plan_store(const Plan& pl, std::vector<uint64_t>&& sig, uint64_t hash) {
  if (g_plan_cache_entries >= 512) {  // (a host that never repeats itself): the least recently used quarter goes
    std::vector<uint64_t> stamps;
    for (auto& kv : plan_cache())
      for (auto& c : kv.second) stamps.push_back(c->used);
    std::nth_element(stamps.begin(), stamps.begin() + stamps.size() / 4, stamps.end());
    const uint64_t cut = stamps[stamps.size() / 4];
    for (auto it = plan_cache().begin(); it != plan_cache().end();) {
      auto& v = it->second;
      const size_t before = v.size();
      v.erase(std::remove_if(v.begin(), v.end(), [&](const std::unique_ptr<CachedPlan>& c) { return c->used <= cut; }), v.end());
      g_plan_cache_entries -= before - v.size();
      it = v.empty() ? plan_cache().erase(it) : std::next(it);
    }
  }
  auto cp = std::make_unique<CachedPlan>();
  cp->used = ++g_plan_clock;
  cp->sig = std::move(sig);
  cp->d = pl.d;
  plan_cache()[hash].push_back(std::move(cp));
  ++g_plan_cache_entries;
}

static const CachedPlan* plan_find(const std::vector<uint64_t>& sig, uint64_t hash) {
  auto it = plan_cache().find(hash);
  if (it == plan_cache().end()) return nullptr;
  for (const auto& cp : it->second)
    if (cp->sig == sig) {
      cp->used = ++g_plan_clock;
      return cp.get();
    }
  return nullptr;
}

static void plan_instantiate(const CachedPlan& cp, Plan& pl) {
  for (const auto& r : cp.d.dlogistic) apply_dlogistic(pl, r.first, r.second);
  pl.d = cp.d;
}

bool plan_cache_take(Plan& pl, PlanKey& key) {
  const CachedPlan* hit = nullptr;
  if (plan_cache_on()) {
    plan_signature(pl, key.sig);
    key.hash = sig_hash(key.sig);
    hit = plan_find(key.sig, key.hash);
  }
  ++(hit ? g_plan_cache_hits : g_plan_cache_misses);
  if (hit) plan_instantiate(*hit, pl);
  return hit != nullptr;
}

void plan_cache_store(const Plan& pl, PlanKey&& key) {
  if (plan_cache_on()) plan_store(pl, std::move(key.sig), key.hash);
}

}  // namespace to
