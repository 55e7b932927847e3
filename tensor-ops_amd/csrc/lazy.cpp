// Deferred execution of the `class Tensor` method stream, and its fusion into the GEMM kernels' epilogues.
//
// Why this exists.  The reference's `Network` is `{Sing ps, TOp, Prod t ps}` -- no activation tags
// (src/TensorOps/Learn/NeuralNet/FeedForward.hs:57-61) -- and `trainNetwork` only ever calls `gradTOp` on
// opaque closures (FeedForward.hs:131-148, src/TensorOps/Types.hs:127-132).  All a backend sees is a stream
// of class-method calls (src/TensorOps/Types.hs:52-109): gmul, liftT, sumT, scaleT, transp, sumRows, mapRows.
// Run one kernel per call and the MNIST step is 29 launches.  The methods are pure and their results are
// immutable values, so inside a fusion scope (to_memo_begin .. to_memo_end) they are RECORDED instead: each
// call returns a handle with a shape and no storage, and when a result is demanded (a download, `to_force`,
// `to_copy_into`, the end of the scope for results the host still holds) the recorded graph is planned:
//
//   gmul -> (+ unbatched vector) -> logistic                  one GEMM launch, bias and activation in its epilogue
//   gmul -> scale / p - r*g with p of the result's shape     alpha, beta*Cin in the epilogue (the SGD update)
//   d * logistic'(z) where h = logistic(z) is in the graph    rewritten to d * h(1-h): z need not be stored
//   the row-local subgraph between z = gmul+bias [B x N<=16] and dz (softmax, log, dot, ... and their
//   cotangents, whatever order the host's AD produced)        evaluated on the host on random rows and compared
//                                                             with the closed forms the small-GEMM kernel carries
//                                                             (softmax>>>crossEntropy, logistic>>>squaredError):
//                                                             the loss head of that launch
//   gmul(W^T, dz) -> * h(1-h)                                 the tail of the loss-head launch
//   gmul_batch_sum(dz, a) next to batch_sum(dz)               the weight-gradient GEMM with its row sums
//   two independent weight-gradient GEMMs                     one launch (gemm_small_pair_kernel)
//   to_copy_into(dst, result)                                 the result is produced in dst
//
// Anything that matches no rule runs through the same eager implementation as outside a scope, so the recorded
// graph always has a correct execution; rules only remove launches and intermediate stores.  Results nobody
// demands are never computed (the reference gets this from Haskell's laziness: the input's cotangent that
// `trainNetwork` drops with `tail'`, FeedForward.hs:142).
//
// Where it lives.  This file: recording, scopes and the memo table, handle helpers, `flush`, `ensure*`, the write hazards.
// lazy_plan.cpp plans a flush, lazy_cache.cpp keeps plans by signature, lazy_exec.cpp runs one (lazy_plan.hpp is what they
// share).  Everything the planner decides is ONE record (Decisions) that names operands by position, "input k of node i";
// a cached plan is that record, bound by position: a flush that finds its signature in the cache and the flush that was
// planned execute from the same object.  What has run and what exists is execution state and belongs to Exec.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <unordered_map>

#include "lazy_plan.hpp"

namespace to {

static Node* g_head = nullptr;
static uint64_t g_seq = 0;
int64_t g_lazy_stats[6] = {0, 0, 0, 0, 0, 0};

static uint64_t this_thread() {
  static std::atomic<uint64_t> next{1};
  static thread_local uint64_t id = next++;
  return id;
}

int64_t lazy_stat(int which) { return which >= 0 && which < 6 ? g_lazy_stats[which] : 0; }

void retain_int(to_tensor t) {
  t->refs.fetch_add(1);
  t->int_refs++;
}
void release_int(to_tensor t) {
  t->int_refs--;
  release(t);
}

static void unlink(Node* n) {
  if (n->prev) n->prev->next = n->next;
  else if (g_head == n) g_head = n->next;
  if (n->next) n->next->prev = n->prev;
  n->prev = n->next = nullptr;
}

// frees t's node (the value exists now, or the handle died): releases the inputs it kept alive
void lazy_drop_node(to_tensor t) {
  Node* n = t->node;
  if (!n) return;
  t->node = nullptr;
  unlink(n);
  std::vector<to_tensor> in;
  in.swap(n->in);
  if (n->d.f) expr_release(n->d.f);
  delete n;
  for (to_tensor x : in) release_int(x);
}

// ---- fusion scope: thread-local depth + CSE memo -----------------------------------------------------------------
struct Scope {
  int depth = 0;
  std::unordered_map<MemoKey, to_tensor, MemoKeyHash> memo;
};
// (heap-allocated and never freed: to_shutdown may walk the list after the thread is gone; a thread that exits
//  drops its memo table)
struct ScopeOwner {
  Scope* s = new Scope();
  ~ScopeOwner();
};
static Scope& scope() {
  static thread_local ScopeOwner o;
  return *o.s;
}
// the scopes of all threads that ever opened one, so that to_shutdown can drop their memo tables
static std::vector<Scope*>& all_scopes() {
  static std::vector<Scope*> v;
  return v;
}

// The deferral switch: TOPS_LAZY gives the default, to_set_lazy overrides it FOR THE CALLING THREAD (scopes and memo
// tables are per thread too: one thread turning fusion off for a call must not change what another thread's open scope
// records).
static int& lazy_override() {
  static thread_local int v = -1;
  return v;
}
static bool lazy_enabled() {
  static const int dflt = [] { const char* e = getenv("TOPS_LAZY"); return e ? atoi(e) : 1; }();
  const int o = lazy_override();
  return (o >= 0 ? o : dflt) != 0;
}
int lazy_set(int on) {
  const int prev = lazy_enabled() ? 1 : 0;
  lazy_override() = on ? 1 : 0;
  return prev;
}

bool lazy_active() { return lazy_enabled() && scope().depth > 0; }

to_tensor memo_find(const MemoKey& key) {
  Scope& s = scope();
  if (s.depth == 0) return nullptr;
  auto it = s.memo.find(key);
  if (it == s.memo.end()) return nullptr;
  retain(it->second);
  return it->second;
}

void memo_put(const MemoKey& key, to_tensor t) {
  Scope& s = scope();
  if (s.depth == 0) return;
  auto it = s.memo.find(key);
  if (it != s.memo.end()) release_int(it->second);
  retain_int(t);
  s.memo[key] = t;
}

static void memo_clear(Scope& s) {
  std::unordered_map<MemoKey, to_tensor, MemoKeyHash> m;
  m.swap(s.memo);
  for (auto& kv : m) release_int(kv.second);
}

ScopeOwner::~ScopeOwner() {
  std::lock_guard<std::recursive_mutex> guard(lock());
  memo_clear(*s);
  s->depth = 0;
}

void scope_begin() {
  Scope& s = scope();
  if (s.depth == 0) add_unique(all_scopes(), &s);
  ++s.depth;
}

void scope_end() {
  Scope& s = scope();
  TO_CHECK(s.depth > 0, TO_ERR_STATE, "to_memo_end without to_memo_begin");
  // Closing a scope demands nothing.  A handle the host still holds stays deferred and is produced if and when
  // it is asked for: under a garbage collector "still held" says nothing about "still wanted" -- every intermediate
  // of a step is reachable from the Haskell heap until the finaliser of its ForeignPtr has run, and launching those
  // here would re-run the whole step unfused.
  if (--s.depth == 0) memo_clear(s);
}

void scope_reset_all() {
  for (Scope* s : all_scopes()) {
    memo_clear(*s);
    s->depth = 0;
  }
  // handles that are still deferred keep their nodes; they die with their handles
}

to_tensor lazy_record(const NodeDesc& d, int n_in, const to_tensor* in, int rank, const int64_t* dims,
                      int64_t batch, int dtype) {
  to_tensor t = new_deferred(rank, dims, batch, dtype);
  auto* n = new Node();
  n->d = d;
  if (n->d.f) expr_retain(n->d.f);
  n->seq = ++g_seq;
  n->owner = this_thread();
  n->in.assign(in, in + n_in);
  for (to_tensor x : n->in) retain_int(x);
  n->out = t;
  n->next = g_head;
  if (g_head) g_head->prev = n;
  g_head = n;
  t->node = n;
  g_lazy_stats[0]++;
  return t;
}

bool lazy_node_of(to_tensor t, NodeDesc* d, std::vector<to_tensor>* in) {
  if (t->ptr || t->view_base || !t->node) return false;
  *d = t->node->d;
  *in = t->node->in;
  return true;
}

// ---- handles and memory ---------------------------------------------------------------------------------------------
// the pending node a handle's value comes from (nullptr: the value exists; a pending view gets resolved here)
void resolve_view(to_tensor t) {
  to_tensor_s* b = t->view_base;
  if (!b || !b->ptr) return;
  t->buf = b->buf;
  if (t->buf) t->buf->refs.fetch_add(1);
  t->ptr = b->at(t->view_off);
  t->view_base = nullptr;
  for (size_t i = 0; i < b->dviews.size(); ++i)
    if (b->dviews[i] == t) {
      b->dviews[i] = b->dviews.back();
      b->dviews.pop_back();
      break;
    }
  release_int(b);
}

Node* producer(to_tensor t) {
  if (t->ptr) return nullptr;
  if (t->view_base) {
    if (t->view_base->ptr) {
      resolve_view(t);
      return nullptr;
    }
    TO_CHECK(t->view_base->node != nullptr, TO_ERR_STATE, "deferred view of a handle without a recorded op");
    return t->view_base->node;
  }
  TO_CHECK(t->node != nullptr, TO_ERR_STATE, "handle has neither storage nor a recorded op");
  return t->node;
}

static bool is_live(to_tensor t) { return t->refs.load() > t->int_refs; }
// can the host still ask for this value -- through the handle, or through a view of it that it holds?
static bool host_reachable(to_tensor t) {
  if (is_live(t)) return true;
  for (to_tensor_s* v : t->dviews)
    if (is_live(v)) return true;
  return false;
}

// does `in` denote exactly the value of handle h, element for element in the same order?
bool same_value_layout(to_tensor in, to_tensor h) {
  if (in == h) return true;
  if (in->view_base != h || in->view_off != 0 || in->rank != h->rank || in->batch != h->batch) return false;
  for (int i = 0; i < h->rank; ++i)
    if (in->dims[i] != h->dims[i] || (h->dims[i] != 1 && in->strides[i] != h->strides[i])) return false;
  return h->batch <= 1 || in->bstride == h->bstride;
}

// byte range a materialised handle can touch
void mem_range(to_tensor t, const char** lo, const char** hi) {
  int64_t last = 0;
  for (int i = 0; i < t->rank; ++i)
    if (t->dims[i] > 0) last += (t->dims[i] - 1) * t->strides[i];
  if (t->batch > 1) last += (t->batch - 1) * t->bstride;
  *lo = static_cast<const char*>(t->ptr);
  *hi = *lo + (last + 1) * (int64_t)t->esize();
  if (t->total() == 0) *hi = *lo;
}
bool overlaps(to_tensor a, to_tensor b) {
  if (!a->ptr || !b->ptr) return false;
  const char *al, *ah, *bl, *bh;
  mem_range(a, &al, &ah);
  mem_range(b, &bl, &bh);
  return al < bh && bl < ah;
}

// ---- one flush -----------------------------------------------------------------------------------------------------------
static void flush(const std::vector<to_tensor>& demand, const std::vector<std::pair<to_tensor, to_tensor>>& copies) {
  const auto t_begin = std::chrono::steady_clock::now();
  struct Timer {
    std::chrono::steady_clock::time_point t0;
    ~Timer() { g_lazy_stats[5] += std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count(); }
  } timer{t_begin};
  std::vector<to_tensor> roots = demand;
  for (auto& c : copies) roots.push_back(c.second);
  TO_CHECK(gemm_small_chain_status() == 0, TO_ERR_HIP,
           "a grid barrier of a chained step launch timed out (code " + std::to_string(gemm_small_chain_status()) +
               "): the results of that step are invalid; set TOPS_STEP_CHAIN=0");
  TO_CHECK(gemm_t32_take_failure() == 0, TO_ERR_HIP,
           "the joined forward + loss-head launch gave up waiting for a row block's tiles (are CUs masked below one round of the "
           "grid?): the outputs of that launch are invalid; the joined form is off for the rest of this process (TOPS_STEP_SEAM=0 "
           "turns it off from the start)");
  TO_CHECK(gemm_small_seam_take_failure() == 0, TO_ERR_HIP,
           "the joined forward + loss-head launch (TOPS_STEP_SEAM) gave up waiting for a row block: the outputs of that launch "
           "are invalid; the seam is off for the rest of this process");
  Plan pl;
  collect(pl, roots);
  if (pl.ns.empty()) return;
  g_lazy_stats[3]++;
  for (to_tensor t : demand) {
    const int i = pn_of(pl, t);
    if (i >= 0) pl.ns[i].demanded = true;
  }
  for (auto& c : copies) {
    const int i = pn_of(pl, c.second);
    if (i < 0) continue;
    pl.ns[i].copy_dst = c.first;  // (lazy_copy_into passes each deferred result once, never a view)
  }
  // The plan holds a reference to every handle it touches until it is done.  A handle in it may otherwise die midway:
  // resolving a deferred view releases the view's reference to its base (an executed `gmul` whose only holder was its
  // `transp` view), and dropping one node releases the inputs it kept alive -- while `finish` and `pl.ns` still point there.
  // (Inside a scope the memo table used to hide this; values demanded after the scope closed do not have that cover.)
  // (library-side references: they do not make a handle look held by the host)
  struct Held {
    std::vector<to_tensor> v;
    ~Held() {
      for (to_tensor h : v) release_int(h);
    }
  } held;
  for (PN& pn : pl.ns) {
    retain_int(pn.h);
    held.v.push_back(pn.h);
  }
  PlanKey key;
  if (!plan_cache_take(pl, key)) {
    compute_ancestors(pl);
    plan_groups(pl);
    plan_forwarding(pl);
    if (!topo_order(pl)) {
      // ordering readers of a forwarding destination first closed a cycle: give the forwarding up
      std::fill(pl.d.fwd.begin(), pl.d.fwd.end(), 0);
      for (Gr& g : pl.d.gs) {
        g.deps.clear();
        if (g.pair >= 0) pl.d.gs[g.pair].pair = -1, g.pair = -1;
        g.r1 = -1;
        g.r1_members.clear();
      }
      group_deps(pl);
      TO_CHECK(topo_order(pl), TO_ERR_STATE, "internal: recorded graph has a cycle");
    }
    plan_cache_store(pl, std::move(key));
  }
  if (debug_on()) dump_plan(pl);
  g_lazy_stats[4] += std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t_begin).count();
  run_plan(pl);
}

void ensure(to_tensor t) {
  if (t->ptr) return;
  if (producer(t) == nullptr) return;  // a view that could be resolved
  to_tensor base = t->view_base ? t->view_base : t;
  flush({base}, {});
  if (!t->ptr) resolve_view(t);
  TO_CHECK(t->ptr != nullptr, TO_ERR_STATE, "internal: deferred value was not produced");
}

void ensure_all(int n, const to_tensor* ts) {
  std::vector<to_tensor> need;
  for (int i = 0; i < n; ++i)
    if (ts[i] && !ts[i]->ptr && producer(ts[i])) need.push_back(ts[i]->view_base ? ts[i]->view_base : ts[i]);
  if (!need.empty()) flush(need, {});
  for (int i = 0; i < n; ++i)
    if (ts[i] && !ts[i]->ptr) {
      resolve_view(ts[i]);
      TO_CHECK(ts[i]->ptr != nullptr, TO_ERR_STATE, "internal: deferred value was not produced");
    }
}

// live results of `owner` (0: of every thread) that no recorded op consumes
static std::vector<to_tensor> live_sinks(uint64_t owner) {
  std::unordered_map<Node*, char> consumed;
  for (Node* n = g_head; n; n = n->next)
    for (to_tensor x : n->in) {
      if (x->ptr) continue;
      to_tensor_s* b = x->view_base ? x->view_base : x;
      if (b->node) consumed[b->node] = 1;
    }
  std::vector<to_tensor> out;
  for (Node* n = g_head; n; n = n->next)
    if ((owner == 0 || n->owner == owner) && !consumed.count(n) && is_live(n->out)) out.push_back(n->out);
  return out;
}

void lazy_flush_sinks() {
  if (!g_head) return;
  std::vector<to_tensor> s = live_sinks(this_thread());
  if (!s.empty()) flush(s, {});
}

void lazy_flush_all() {
  if (!g_head) return;
  std::vector<to_tensor> s = live_sinks(0);
  if (!s.empty()) flush(s, {});
}

// recorded ops that read memory about to be overwritten, and everything reachable from them that the host can
// still ask for (a handle it holds, or a view of one): they must see the old contents
static std::vector<to_tensor> stale_after_write(int n, const to_tensor* dsts, const std::vector<to_tensor>& except) {
  if (!g_head) return {};
  // the destinations' byte ranges, once; most operands are rejected against their hull
  std::vector<std::pair<const char*, const char*>> dr;
  const char *hull_lo = nullptr, *hull_hi = nullptr;
  for (int i = 0; i < n; ++i) {
    if (!dsts[i]->ptr) continue;
    const char *lo, *hi;
    mem_range(dsts[i], &lo, &hi);
    if (lo == hi) continue;
    dr.emplace_back(lo, hi);
    if (!hull_lo || lo < hull_lo) hull_lo = lo;
    if (!hull_hi || hi > hull_hi) hull_hi = hi;
  }
  if (dr.empty()) return {};
  auto reads_dst = [&](to_tensor x) {
    const char* p = static_cast<const char*>(x->ptr);
    if (p >= hull_hi) return false;
    const char *lo, *hi;
    mem_range(x, &lo, &hi);
    if (hi <= hull_lo) return false;
    for (auto& r : dr)
      if (lo < r.second && r.first < hi) return true;
    return false;
  };
  // pending nodes in recording order (the list is newest first)
  std::vector<Node*> nodes;
  for (Node* q = g_head; q; q = q->next) nodes.push_back(q);
  bool sorted = true;
  for (size_t i = 1; i < nodes.size() && sorted; ++i) sorted = nodes[i - 1]->seq > nodes[i]->seq;
  if (sorted) std::reverse(nodes.begin(), nodes.end());
  else std::sort(nodes.begin(), nodes.end(), [](const Node* a, const Node* b) { return a->seq < b->seq; });
  static uint64_t g_write_epoch = 0;
  const uint64_t epoch = ++g_write_epoch;  // (marks "hit" nodes in Node::write_mark: pn_of's plan_epoch is not touched)
  bool any = false;
  for (Node* q : nodes) {
    bool h = false;
    for (to_tensor x : q->in) {
      if (x->ptr) {
        h = reads_dst(x);
      } else {
        to_tensor_s* b = x->view_base ? x->view_base : x;
        h = b->node && b->node->write_mark == epoch;
      }
      if (h) break;
    }
    if (h) {
      q->write_mark = epoch;
      any = true;
    }
  }
  std::vector<to_tensor> out;
  if (!any) return out;
  for (Node* q : nodes)
    if (q->write_mark == epoch && host_reachable(q->out) &&
        std::find(except.begin(), except.end(), q->out) == except.end())
      out.push_back(q->out);
  return out;
}

void before_write(to_tensor t) {
  if (!g_head || !t->ptr) return;
  std::vector<to_tensor> s = stale_after_write(1, &t, {});
  if (!s.empty()) flush(s, {});
}

void lazy_copy_into(int n, const to_tensor* dsts, const to_tensor* srcs) {
  std::vector<std::pair<to_tensor, to_tensor>> pending;
  std::vector<to_tensor> psrc;
  for (int i = 0; i < n; ++i) {
    ensure(dsts[i]);
    dsts[i]->id = fresh_id();  // new contents
    if (!srcs[i]->ptr && srcs[i]->node && std::find(psrc.begin(), psrc.end(), srcs[i]) == psrc.end()) {
      pending.push_back({dsts[i], srcs[i]});
      psrc.push_back(srcs[i]);
    }
  }
  if (g_head) {
    std::vector<to_tensor> stale = stale_after_write(n, dsts, psrc);
    // (only the sources and what must read the old contents first: other deferred values the host holds are not
    //  demanded by this call -- under a garbage collector "held" does not mean "wanted", see scope_end)
    if (!pending.empty() || !stale.empty()) flush(stale, pending);
  }
  // sources that already existed
  std::vector<std::unique_ptr<Holder>> keep;
  std::vector<const void*> sp;
  std::vector<void*> dp;
  std::vector<int64_t> dw;
  for (int i = 0; i < n; ++i) {
    bool was_pending = false;
    for (auto& c : pending) was_pending = was_pending || (c.first == dsts[i] && c.second == srcs[i]);
    if (was_pending || dsts[i]->total() == 0) continue;
    ensure(srcs[i]);
    keep.emplace_back(new Holder(contiguous(srcs[i])));
    sp.push_back(keep.back()->t->ptr);
    dp.push_back(dsts[i]->ptr);
    dw.push_back(dsts[i]->total() * (int64_t)dsts[i]->esize() / 4);
  }
  for (size_t b = 0; b < sp.size(); b += 16) {
    const int m = (int)std::min<size_t>(16, sp.size() - b);
    describe_other();
    launch_multi_copy(m, sp.data() + b, dp.data() + b, dw.data() + b, S());
  }
}

}  // namespace to
