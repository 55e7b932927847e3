#include "gemm_route.hpp"

#include "api_util.hpp"

namespace to {

// A sub-block of the output (rows [r0, r0+m), columns [c0, c0+n)) as a problem of its own.
static GemmProblem gemm_block(const GemmProblem& p, int64_t r0, int64_t m, int64_t c0, int64_t n) {
  GemmProblem q = p;
  const int64_t es = p.dtype == TO_F64 ? 8 : 4;
  auto adv = [es](const void* ptr, int64_t elems) -> const void* {
    return ptr ? static_cast<const void*>(static_cast<const char*>(ptr) + elems * es) : nullptr;
  };
  q.M = m; q.N = n;
  q.A = adv(p.A, r0 * p.a_sm);
  q.B = adv(p.B, c0 * p.b_sn);
  q.C = const_cast<void*>(adv(p.C, r0 * p.c_sm + c0));
  q.Cin = adv(p.Cin, r0 * p.c_sm + c0);
  q.bias = adv(p.bias, c0);
  q.dact = adv(p.dact, r0 * p.c_sm + c0);
  return q;
}

// The plan's last question: which tiled kernel gets a (non-empty, unsplit) problem none of the special shapes claimed.
static GemmFamily gemm_tiled_family(const GemmProblem& p) {
  const bool sliver = p.K >= 256 && p.M * p.N >= 256 && gemm_small_can(p) &&
                      ((p.M + 15) / 16) * ((p.N + 15) / 16) * p.batch <= 4096;
  if (gemm_mfma_worthwhile(p) && gemm_small_applicable(p)) return GEMM_SMALL;  // few tiles, long K
  if (gemm_mfma_worthwhile(p) && (p.reduce_batch || p.batch <= 65535)) return p.dtype == TO_F64 ? GEMM_F64 : GEMM_MFMA;
  // a sliver (fewer than 8 rows or columns) with a long K -- e.g. the border strip of a split: one thread per
  // output element would walk K serially (4 x 4096 x 4096: 0.95 ms); the small-GEMM kernel splits K
  if (sliver) return GEMM_SMALL;
  return GEMM_NAIVE;
}

// Large GEMMs whose extents are no multiple of the 256x256 (fp64: 256x128) tile, or whose tile count is no multiple of
// the 256 CUs: the fast full-tile kernel gets the largest block of (nearly) WHOLE ROUNDS of tiles, the two border
// strips go their own way (smaller tiles, split-K, the small-GEMM kernel).  A ragged last round of big tiles
// costs a whole round: 4100x4096x4096 took 2.38 ms against 0.95 ms for 4096^3.
// A K that is no multiple of the 16-deep k-tile puts EVERY tile on the guarded (bounds-checked, scalar-load) path:
// 1000^3 ran at 25 TF.  Run the multiple-of-16 part unguarded and add the K tail (< 16) in a second, tiny launch
// (C = alpha A2.B2 + 1 C).  Only for linear epilogues; the summation order changes within the 1e-5 bar.
void gemm_plan(const GemmProblem& p, GemmLeaves& out, bool sub) {
  if (p.M == 0 || p.N == 0 || p.batch == 0) return;
  TO_CHECK(p.M <= 2147483647LL && p.N <= 2147483647LL && p.K <= 2147483647LL, TO_ERR_SHAPE,
           "collapsed GEMM extent exceeds 2^31-1");
  // one extent is 1: matVec / vecMat / an outer product beyond the small-GEMM kernel's range -- HBM-bound streaming kernels
  if (gemv_form(p, true)) return out.push(GEMM_GEMV, p, sub);
  {   // (development builds, TOPS_T32_FIRST=1: the four-wave 32x32-tile kernel ahead of the wave-split one, for A/B runs)
    static const int t32_first = [] { const char* e = ab_getenv("TOPS_T32_FIRST"); return e ? atoi(e) : 0; }();
    if (t32_first && gemm_t32_applicable(p)) return out.push(GEMM_T32, p, sub);
  }
  // short K, B small enough to live in LDS, a long stream of rows (config 5): the barrier-free streaming kernel -- ahead of the
  // wave-split kernel, whose rule for "more than 1,024 tiles the big tiles do not fit" would take these too (0.150 -> 0.217 ms)
  if (gemm_skinnyk_applicable(p)) return out.push(GEMM_SKINNYK, p, sub);
  if (gemm_skinnyk64_applicable(p)) return out.push(GEMM_SKINNYK64, p, sub);
  // a few hundred 64x64 tiles: the K loop split over the waves of each tile's workgroup (K tails included)
  // ... on the tile shape whose count fits the CUs: 48x48 / 48x64 / 64x48 / 80x80 where that beats the 64x64 routes (768^3: 256
  // tiles of 48x48 instead of 144 of 64x64 split three ways)
  if (gemm_kw16_applicable(p)) return out.push(GEMM_KW16, p, sub);
  if (gemm_kw_applicable(p)) return out.push(GEMM_KW, p, sub);
  if (gemm_kw64_applicable(p)) return out.push(GEMM_KW64, p, sub);
  if (p.K % 16 != 0 && p.K >= 128 && p.M * p.N >= 65536 && !p.reduce_batch && !p.rowsum && !p.loss_rows && p.act == 0 &&
      !p.dact) {
    const int64_t es = p.dtype == TO_F64 ? 8 : 4, K0 = p.K / 16 * 16;
    GemmProblem head = p, tail = p;
    head.K = K0;
    head.bias = nullptr;  // the bias belongs to the launch that finishes the element
    tail.K = p.K - K0;
    tail.A = static_cast<const char*>(p.A) + K0 * p.a_sk * es;
    tail.B = static_cast<const char*>(p.B) + K0 * p.b_sk * es;
    tail.Cin = p.C;
    tail.beta = 1.0;
    gemm_plan(head, out, true);
    gemm_plan(tail, out, true);
    return;
  }
  const bool f64 = p.dtype == TO_F64;
  auto full_rounds = [f64](const GemmProblem& q) { return f64 ? gemm_f64_w4_full_rounds(q) : gemm_w4_full_rounds(q); };
  const int64_t TNW = f64 ? 128 : 256;  // tile width (fp64: 256 x 128 tiles)
  // ragged, but whole rounds of tiles with its edge tiles
  if (!f64 && gemm_w4_edge_whole(p) && gemm_tiled_family(p) == GEMM_MFMA) return out.push(GEMM_MFMA, p, sub);
  if (!p.reduce_batch && !p.rowsum && !p.loss_rows && p.M >= 256 && p.N >= 256 && !full_rounds(p)) {
    const int64_t tm = p.M / 256, tn = p.N / TNW;
    int64_t best = 0, bm = 0, bn = 0;
    for (int64_t dm = 0; dm < 8 && dm < tm; ++dm)
      for (int64_t dn = 0; dn < 8 && dn < tn; ++dn) {
        const int64_t t = (tm - dm) * (tn - dn) * p.batch;
        if (t > best && full_rounds(gemm_block(p, 0, (tm - dm) * 256, 0, (tn - dn) * TNW))) { best = t; bm = tm - dm; bn = tn - dn; }
      }
    // worth it when the block carries at least half of the work
    if (best > 0 && 2 * bm * bn * 256 * TNW >= p.M * p.N) {
      const GemmProblem main = gemm_block(p, 0, bm * 256, 0, bn * TNW);
      if (full_rounds(main)) {
        gemm_plan(main, out, true);
        if (bn * TNW < p.N) gemm_plan(gemm_block(p, 0, p.M, bn * TNW, p.N - bn * TNW), out, true);       // right strip
        if (bm * 256 < p.M) gemm_plan(gemm_block(p, bm * 256, p.M - bm * 256, 0, bn * TNW), out, true);  // bottom strip
        return;
      }
    }
  }
  // Mid sizes whose extents are no multiple of 4 (multiples of 4 run whole on the pinned 128-tile kernel, edge tiles
  // included): the block of whole 128x128 tiles goes to that kernel, the two border strips their own way (slivers
  // with a long K: the small-GEMM kernel).  Otherwise every tile is on the guarded scalar-load path.
  if (!f64 && p.batch == 1 && !p.reduce_batch && !p.rowsum && !p.loss_rows && p.K % 16 == 0 && p.M >= 384 && p.N >= 384 &&
      (p.M % 4 != 0 || p.N % 4 != 0) && p.beta == 0.0 && p.alpha == 1.0 && !p.bias && !p.dact && p.act == 0) {
    const int64_t bm = p.M / 128, bn = p.N / 128;
    if (bm * bn >= 16 && bm * bn <= 288 && 4 * bm * bn * 128 * 128 >= 3 * p.M * p.N) {
      gemm_plan(gemm_block(p, 0, bm * 128, 0, bn * 128), out, true);
      if (bn * 128 < p.N) gemm_plan(gemm_block(p, 0, p.M, bn * 128, p.N - bn * 128), out, true);          // right strip
      if (bm * 128 < p.M) gemm_plan(gemm_block(p, bm * 128, p.M - bm * 128, 0, bn * 128), out, true);     // bottom strip
      return;
    }
  }
  const GemmFamily f = gemm_tiled_family(p);  // (small: latency-bound shapes, in-workgroup split-K, no LDS staging)
  TO_CHECK(f != GEMM_F64 || (!p.bias && !p.act && !p.dact), TO_ERR_STATE,
           "internal: fused epilogue routed to the tiled fp64 kernel");
  out.push(f, p, sub);
}

// The only place that maps a family to its launcher on run_gemm's behalf.
void run_gemm(const GemmProblem& p) {
  GemmLeaves plan;
  gemm_plan(p, plan);
  for (int i = 0; i < plan.n; ++i) {
    const GemmProblem& q = *plan.problem[i];
    switch (plan.family[i]) {
      case GEMM_GEMV: launch_gemv(q, S()); break;
      case GEMM_T32: launch_gemm_t32(q, S()); break;
      case GEMM_SKINNYK: launch_gemm_skinnyk(q, S()); break;
      case GEMM_SKINNYK64: launch_gemm_skinnyk64(q, S()); break;
      case GEMM_KW16: launch_gemm_kw16(q, S()); break;
      case GEMM_KW: launch_gemm_kw(q, S()); break;
      case GEMM_KW64: launch_gemm_kw64(q, S()); break;
      case GEMM_SMALL: launch_gemm_small(q, S()); break;
      case GEMM_MFMA: launch_gemm_mfma(q, S()); break;
      case GEMM_F64: launch_gemm_f64(q, S()); break;
      case GEMM_NAIVE: launch_gemm_naive(q, S()); break;
    }
  }
}

// ---- the predicates ----------------------------------------------------------------------------------------------------
// Both are asked BEFORE a caller settles a problem's epilogue (the planner's fusion, the stack entries), and the launches --
// through them result bits and speed -- depend on their answers: they answer as they always have.  Neither can be read off
// gemm_plan's leaves without changing an answer; where they part from the plan, once:
//  - gemm_small_route is not "the plan says small": its callers launch the small-GEMM kernel themselves, AHEAD of the plan's
//    order (run_gemm_small_first), so it holds for problems the plan hands to gemv (standalone form), skinnyk, kw16, kw, kw64 or
//    naive.  It asks gemv_form(p) where the plan asks gemv_form(p, true): plan says gemv for a product that stands alone,
//    predicate says small, kept.
//  - plan says kw16 / kw (one leaf, epilogue carried) where gemm_tiled_family says naive: gemm_epilogue_ok says no, kept.
//  - plan says naive (the kernel carries the epilogue): gemm_epilogue_ok says no, kept.
//  - plan says small for an fp64 problem gemm_small_route does not hold for (batched, or a sliver; carried):
//    gemm_epilogue_ok says no, kept.
//  - plan says gemv through the standalone form only: gemm_epilogue_ok asks gemv_form(p), as gemm_small_route does, and
//    does not take the plan's gemv for a yes, kept.
//  - plan splits (K tail, strips) an fp32 problem whose gemm_tiled_family is small / mfma: gemm_epilogue_ok answers for the
//    whole problem, yes -- every fp32 kernel a strip or a tail may land on carries the epilogue.
// What they do share with the plan is gemm_tiled_family, its last question.  Making either less conservative is a
// performance change, to be measured as one.
bool gemm_small_takes(const GemmProblem& p) {
  const int64_t t64 = ((p.M + 63) / 64) * ((p.N + 63) / 64);
  return gemm_small_can(p) && t64 < 200;
}

bool gemm_small_route(const GemmProblem& p) {
  if (p.M == 0 || p.N == 0 || p.K == 0 || p.batch != 1 || p.reduce_batch) return false;
  if (gemv_form(p)) return false;   // (a large matVec / vecMat / outer product: gemv.hip, through run_gemm)
  // (a few tiles under a very long K -- a weight gradient over a data set, 300 x 60000 x 784: one workgroup a tile here whatever K
  //  is, 400 us; 291 split over workgroups in gemm_kwave.hip, which carries alpha / beta C / bias / activation but no row sums)
  if (p.K >= 8192 && !p.rowsum && !p.loss_rows && !p.tail_out && gemm_kw_long_k(p)) return false;
  return gemm_small_takes(p);
}

// The fused elementwise epilogue (alpha, beta*Cin, bias, act, dact) exists in the small-GEMM kernel (both element
// types), the tiled fp32 kernel and the one-thread-per-element fallback (where border strips and K tails of a problem
// the plan splits may land) and both wave-split kernels (gemm_kwave*.hip); the tiled fp64 kernel has alpha/beta only.
bool gemm_epilogue_ok(const GemmProblem& p) {
  if (p.M == 0 || p.N == 0 || p.K == 0 || p.batch == 0) return false;
  if (gemm_small_route(p) || gemm_skinnyk_applicable(p) || gemm_skinnyk64_applicable(p) || gemv_form(p)) return true;
  if (p.dtype == TO_F64) return gemm_kw64_applicable(p);
  const GemmFamily f = gemm_tiled_family(p);
  return f == GEMM_SMALL || f == GEMM_MFMA;
}

void run_gemm_small_first(const GemmProblem& p) {
  if (gemm_small_route(p)) launch_gemm_small(p, S());
  else run_gemm(p);
}

// The problem the debug query asks about: operands laid out as gmul lays out a contiguous / transposed one.
static GemmProblem route_query_problem(int dtype, int64_t m, int64_t n, int64_t k, int64_t batch, int reduce_batch,
                                       int a_transposed, int b_transposed, int epilogue) {
  // operands that nothing dereferences: distinct, 16-byte aligned, far enough apart for every sub-block's offsets
  auto dummy = [](int i) { return reinterpret_cast<void*>((uintptr_t)(i + 1) << 44); };
  GemmProblem p{};
  p.dtype = dtype;
  p.A = dummy(0); p.B = dummy(1); p.C = dummy(2);
  p.M = m; p.N = n; p.K = k;
  p.a_sm = a_transposed ? 1 : k; p.a_sk = a_transposed ? m : 1;
  p.b_sk = b_transposed ? 1 : n; p.b_sn = b_transposed ? k : 1;
  p.c_sm = n;
  p.batch = batch;
  p.reduce_batch = reduce_batch ? 1 : 0;
  p.a_sb = batch > 1 ? m * k : 0;
  p.b_sb = batch > 1 ? k * n : 0;
  p.c_sb = batch > 1 && !reduce_batch ? m * n : 0;
  p.alpha = 1.0;
  p.beta = epilogue & TO_GEMM_EPI_BETA ? 1.0 : 0.0;
  p.Cin = epilogue & TO_GEMM_EPI_BETA ? dummy(3) : nullptr;
  p.bias = epilogue & TO_GEMM_EPI_BIAS ? dummy(4) : nullptr;
  p.act = epilogue & TO_GEMM_EPI_ACT ? 1 : 0;
  p.dact = epilogue & TO_GEMM_EPI_DACT ? dummy(5) : nullptr;
  p.rowsum = epilogue & TO_GEMM_EPI_ROWSUM ? dummy(6) : nullptr;
  return p;
}

}  // namespace to

// ---- the debug query (include/tensorops_hip.h) ---------------------------------------------------------------------------
extern "C" to_status to_gemm_route_query(int dtype, int64_t m, int64_t n, int64_t k, int64_t batch, int reduce_batch,
                                         int a_transposed, int b_transposed, int epilogue, int capacity, int* families,
                                         int* n_leaves, int* epilogue_ok, int* small_route, int* split_workspace) {
  using namespace to;
  API_BEGIN
  require_init();
  NONNULL(n_leaves);
  TO_CHECK(dtype == TO_F32 || dtype == TO_F64, TO_ERR_ARG, "unknown dtype");
  TO_CHECK(m >= 0 && n >= 0 && k >= 0 && batch >= 1, TO_ERR_ARG, "gemm_route_query: negative extent or batch < 1");
  TO_CHECK(capacity >= 0 && (capacity == 0 || families), TO_ERR_ARG, "gemm_route_query: null families");
  TO_CHECK((epilogue & ~(TO_GEMM_EPI_BIAS | TO_GEMM_EPI_ACT | TO_GEMM_EPI_DACT | TO_GEMM_EPI_BETA | TO_GEMM_EPI_ROWSUM)) == 0,
           TO_ERR_ARG, "gemm_route_query: unknown epilogue bit");
  const GemmProblem p = route_query_problem(dtype, m, n, k, batch, reduce_batch, a_transposed, b_transposed, epilogue);
  GemmLeaves plan;
  try {
    gemm_plan(p, plan);
    *n_leaves = plan.n;
  } catch (const Error& e) {   // (what run_gemm would refuse: an extent past 2^31-1, a fused epilogue on the tiled fp64 kernel)
    g_err = e.what();
    *n_leaves = -1;
  }
  for (int i = 0; i < *n_leaves && i < capacity; ++i) families[i] = plan.family[i];
  if (epilogue_ok) *epilogue_ok = gemm_epilogue_ok(p);
  if (small_route) *small_route = gemm_small_route(p);
  if (split_workspace) *split_workspace = xcd_placement_probe();
  API_END
}
