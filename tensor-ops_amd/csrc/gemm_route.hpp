// Which kernel(s) a contraction goes to: the routing decision (gemm_plan, which launches nothing), its executor (run_gemm)
// and the predicates callers ask before they build a problem's epilogue.  DESIGN.md 3.1 is this file's table.
#pragma once
#include <new>
#include <type_traits>

#include "common.hpp"

namespace to {

// The kernel families in the order gemm_plan asks them (include/tensorops_hip.h, TO_GEMM_FAMILY_*).
enum GemmFamily {
  GEMM_GEMV = TO_GEMM_FAMILY_GEMV,            // gemv.hip
  GEMM_T32 = TO_GEMM_FAMILY_T32,              // gemm_t32.hip (development builds, TOPS_T32_FIRST=1 only)
  GEMM_SKINNYK = TO_GEMM_FAMILY_SKINNYK,      // gemm_skinnyk.hip
  GEMM_SKINNYK64 = TO_GEMM_FAMILY_SKINNYK64,  // gemm_skinnyk_f64.hip
  GEMM_KW16 = TO_GEMM_FAMILY_KW16,            // gemm_kw16.hip
  GEMM_KW = TO_GEMM_FAMILY_KW,                // gemm_kwave.hip
  GEMM_KW64 = TO_GEMM_FAMILY_KW64,            // gemm_kwave_f64.hip
  GEMM_SMALL = TO_GEMM_FAMILY_SMALL,          // gemm_small.hip
  GEMM_MFMA = TO_GEMM_FAMILY_MFMA,            // gemm_f32_mfma.hip
  GEMM_F64 = TO_GEMM_FAMILY_F64,              // gemm_f64.hip
  GEMM_NAIVE = TO_GEMM_FAMILY_NAIVE,          // reduce_layout.hip: one thread per output element
};

// A plan's leaves -- one launch each: a kernel family and the (sub-)problem it gets -- in launch order, held inline (no heap
// on any path).  An unsplit problem, the rule by far, is ONE leaf that refers to the caller's problem: nothing is copied, and
// the plan must not outlive that problem.  Only the sub-problems of a split are kept here.  Their storage is raw bytes written
// by placement new: an array of GemmProblem would run 64 constructors (its members have initialisers) in every run_gemm; as
// it is, a run_gemm frame is about 20 KB of which an unsplit problem touches a few words.
// The bound, from gemm_plan's recursion:
//  - the K tail splits once: its head has K % 16 == 0 and its tail K < 16, neither splits along K again, and the tail (K % 16
//    != 0: no whole-rounds block, no 128-tile block) is one leaf;
//  - the 128-tile split is three leaves: its block (at most 288 tiles of 128 x 128, multiples of 4, batch 1: fewer than the 128
//    big tiles a whole-rounds block needs) and its strips (fewer than 128 columns / rows) split no further;
//  - the whole-rounds split: its block is a leaf (whole rounds, same K and epilogue as its parent), its right strip keeps
//    fewer than 8 tile columns, its bottom strip fewer than 8 tile rows, and a strip that splits again hands at least one of
//    them to its own block.  With batch == 1 a corner (fewer than 8 x 8 tiles) is short of the 128 tiles a block needs, so a
//    strip is a chain of at most 7 splits, each a block, a corner and the next strip: 2 * 7 + 1 = 15 leaves, two strips and
//    the block 31, and the K tail makes 32.
// A BATCHED problem counts batch x tiles, so its corners may split again and the recursion alone bounds its leaves only by
// thousands.  The capacity is twice the batch == 1 bound, and a plan past it is REFUSED (TO_ERR_STATE) where the cascade
// would have gone on launching: the one accepted difference besides the earlier fp64 check.  It takes a batched product
// whose strips and corners find whole rounds again and again; the recorded route table (tests/golden/gemm_routes.txt,
// batch 16 included) has four leaves at the most, three as a rule.
struct GemmLeaves {
  static constexpr int CAP = 64;
  int n = 0;
  GemmFamily family[CAP];
  const GemmProblem* problem[CAP];
  void push(GemmFamily f, const GemmProblem& p, bool keep) {
    TO_CHECK(n < CAP, TO_ERR_STATE, "internal: a contraction's plan has more than 64 launches");
    family[n] = f;
    problem[n] = keep ? new (raw + (size_t)n * sizeof(GemmProblem)) GemmProblem(p) : &p;
    ++n;
  }

 private:
  static_assert(std::is_trivially_destructible<GemmProblem>::value && std::is_trivially_copyable<GemmProblem>::value,
                "sub-problems are copied into raw storage and never destroyed");
  alignas(GemmProblem) unsigned char raw[CAP * sizeof(GemmProblem)];
};

// The routing decision: appends what run_gemm launches for p, in launch order (a split's block, right strip, bottom strip; a K
// split's head, then tail).  Launches nothing, allocates nothing, and reads no pointer beyond its alignment bits.
// (sub: p is a temporary of the recursion, to be kept by the plan; callers leave it out.)
void gemm_plan(const GemmProblem& p, GemmLeaves& out, bool sub = false);
// gemm_plan, then each leaf's launcher.
void run_gemm(const GemmProblem& p);

// would run_gemm honour alpha/beta/Cin/bias/act/dact of this problem (every kernel it may pick carries them)?
bool gemm_epilogue_ok(const GemmProblem& p);
// is the problem in the range of the small-GEMM kernel, the only one with rowsum / loss head / tail epilogues?
bool gemm_small_route(const GemmProblem& p);
// Does the small-GEMM kernel -- the only one with every fused epilogue for both element types -- take this one problem?
// (Every caller has batch == 1.  There `gemm_small_applicable(p) ||` in front of this changes nothing: applicable is can,
//  the same tile bound and M * N >= 256 on top, so it implies this.)
bool gemm_small_takes(const GemmProblem& p);
// the small-GEMM kernel where gemm_small_route holds (run_gemm's own order asks other kernels first), else run_gemm
void run_gemm_small_first(const GemmProblem& p);

}  // namespace to
