#pragma once
// The plan of one flush of the recorded class-method stream: what lazy.cpp (recording, flush), lazy_plan.cpp (the planner),
// lazy_cache.cpp (the plan cache) and lazy_exec.cpp (execution) share.  Internal: included by lazy*.cpp only.
#include <algorithm>
#include <memory>
#include <vector>

#include "ops.hpp"

namespace to {

// ---- recorded ops ---------------------------------------------------------------------------------------------
struct Node {
  NodeDesc d;
  uint64_t seq = 0;    // recording order: inputs always have smaller numbers
  uint64_t owner = 0;  // recording thread
  std::vector<to_tensor> in;  // retained (counted in int_refs)
  to_tensor_s* out = nullptr; // the handle that owns this node
  Node *prev = nullptr, *next = nullptr;  // the global list of pending nodes
  uint64_t plan_epoch = 0;  // position in the plan being built (valid while plan_epoch == the plan's epoch)
  uint64_t write_mark = 0;  // stale_after_write's own mark (its own field: a plan may be live when a write hazard is checked)
  int plan_idx = -1;
};

// ---- the plan of one flush ---------------------------------------------------------------------------------------------
struct PN {
  Node* n = nullptr;
  to_tensor h = nullptr;
  std::vector<int> prod;  // per input: producing PN, -1 = the value exists
  std::vector<int> cons;  // distinct consuming PNs
  bool demanded = false;  // must exist in storage of its own after the flush
  to_tensor copy_dst = nullptr;  // to_copy_into destination (a root that need not have storage of its own)
  bool is_const = false;  // every element equals cval (FILL and what is computed from FILLs alone)
  double cval = 0.0;
};

// "input `in` of plan node `node`": how a group names an operand.  A position, not a pointer: the same group binds to the
// handles of whichever flush it is applied to (operand() below), the one that planned it and every later one that finds it
// in the cache alike
struct Ref {
  int node = -1, in = -1;
  explicit operator bool() const { return node >= 0; }
};

struct Gr {
  bool gemm = false;
  std::vector<int> mem;  // members in recording order; those that are no output are never stored
  int anchor = -1, out = -1;
  double alpha = 1.0, beta = 0.0;
  Ref cin, bias, dact;
  int act = 0;       // 1: logistic, 2: tanh
  int dact_kind = 0; // 0: * h (1 - h), 1: * (1 - h^2)
  int rs = -1;  // PN receiving the row sums of the A operand (batch_sum(dz), or p_b - r * that)
  Ref rs_in;
  double rs_alpha = 1.0;
  int loss_kind = 0, loss_node = -1;
  Ref target;
  int tail = -1;  // PN receiving (dz . W) * h(1-h)
  Ref tail_w, tail_h;
  bool wgrad_like = false;
  int pair = -1;          // the other weight-gradient group launched together with this one
  int r1 = -1;            // leader of the rank-1 unit this group belongs to (K = 1 weight gradients of a one-sample
                          // step: all layers' outer-product updates in ONE launch)
  std::vector<int> r1_members;  // on the leader
  std::vector<int> deps;  // groups whose outputs (or whose reads of a forwarding destination) come first
  // a row program (rowprog.cpp): the members are a row-local subgraph hanging off node rp_root, run as ONE compiled kernel
  std::shared_ptr<RowProg> rowprog;
  int rp_root = -1;
  std::vector<int> rp_outs;  // plan nodes whose values the program writes back (parallel to rowprog->outs)
  std::vector<Ref> rp_ext;   // the existing tensors it reads
};

// Everything the planner decides about a flush, and nothing else: the planner fills it (plan_groups, plan_forwarding,
// topo_order), the plan cache keeps a copy of it, execution reads it.  It holds positions only -- no handle, no address, no
// execution state -- so a copy of it IS the plan of any flush with the same signature.
struct Decisions {
  std::vector<Gr> gs;
  std::vector<int> group;   // per node
  std::vector<char> fwd;    // per node: produce it straight into its copy destination
  std::vector<int> order;   // the groups in execution order
  std::vector<std::pair<int, int>> dlogistic;  // rewrite_dlogistic: node i reads the value of node c instead of z
};

struct Plan {
  std::vector<PN> ns;
  uint64_t epoch = 0;
  std::vector<std::vector<uint64_t>> anc;  // ancestor bitsets (over ns)
  int words = 0;
  Decisions d;
  bool is_anc(int a, int of) const { return (anc[of][a >> 6] >> (a & 63)) & 1; }
};

inline to_tensor operand(const Plan& pl, Ref r) { return r ? pl.ns[(size_t)r.node].n->in[(size_t)r.in] : nullptr; }

template <class T>
void add_unique(std::vector<T>& v, const T& x) {
  if (std::find(v.begin(), v.end(), x) == v.end()) v.push_back(x);
}

// lazy.cpp: handles and memory
extern int64_t g_lazy_stats[6];  // recorded, fused launches, elided, flushes, ns spent planning, ns spent in flushes in all
void retain_int(to_tensor t);
void release_int(to_tensor t);
void lazy_drop_node(to_tensor t);  // frees t's node (the value exists now, or the handle died)
void resolve_view(to_tensor t);
Node* producer(to_tensor t);  // the pending node a handle's value comes from (nullptr: the value exists)
bool same_value_layout(to_tensor in, to_tensor h);
void mem_range(to_tensor t, const char** lo, const char** hi);
bool overlaps(to_tensor a, to_tensor b);

inline int pn_of(const Plan& pl, to_tensor t) {
  Node* p = producer(t);
  return p && p->plan_epoch == pl.epoch ? p->plan_idx : -1;
}
inline bool full_like(to_tensor x, to_tensor like) {  // same per-sample shape AND same batch, contiguous
  return same_shape(x, like) && x->batch == like->batch && x->dtype == like->dtype && x->contiguous();
}
inline void dry_plan(const Node* n, GmulPlan& gp) {
  gmul_plan(gp, n->d.lm, n->d.lo, n->d.ln, n->in[0], n->in[1], n->d.reduce, true);
}

// lazy_plan.cpp: the planner
bool debug_on();  // TOPS_LAZY_DEBUG
bool loss_head_match_on();
void collect(Plan& pl, const std::vector<to_tensor>& roots);
void compute_ancestors(Plan& pl);
void apply_dlogistic(Plan& pl, int i, int c);
void group_deps(Plan& pl);
void plan_groups(Plan& pl);
void plan_forwarding(Plan& pl);
bool topo_order(Plan& pl);
void dump_plan(const Plan& pl);

// lazy_cache.cpp: the plan cache
struct PlanKey {
  std::vector<uint64_t> sig;
  uint64_t hash = 0;
};
bool plan_cache_take(Plan& pl, PlanKey& key);  // true: pl.d is the cached record of this signature, its rewrites applied
void plan_cache_store(const Plan& pl, PlanKey&& key);

// lazy_exec.cpp: runs the plan; drops the nodes of the values that exist afterwards
void run_plan(const Plan& pl);
void describe_other();

}  // namespace to
