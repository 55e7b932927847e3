// fp32 GEMM on the bf16 matrix pipe: C[M x N] = alpha A[M x K] B[K x N] (+ beta Cin) (+ bias) (activation), fp32, batch 1, A and
// B in either storage order.  Off unless to_set_gemm_f32_split turns it on.
//
// An fp32 number is the exact sum of three bf16 numbers (24 mantissa bits = 8 + 8 + 8, the same exponent range), and a bf16 x
// bf16 product is exact in the fp32 accumulator of v_mfma_f32_32x32x16_bf16.  So a b = sum over pieces a_p b_q: nine products,
// or six without a1 b2, a2 b1, a2 b2 (each below 2^-24 of a0 b0: ~1e-8 relative in all), on a pipe 16 x the fp32 MFMA's rate by
// the data sheet.  Two launches:
//
//  1. gemm_split_pre_kernel, ONE launch for both operands (blockIdx.y), writes the three planes of each into pool scratch.
//      * The split TRUNCATES: a0 = the top 16 bits of x, a1 = the top 16 bits of x - a0, a2 = x - a0 - a1.  Both differences are
//        exact in fp32 (Sterbenz-like: each removes the leading 8 bits), a2 has at most 8 significant bits left, and |a0| <= |x|,
//        so NO piece can overflow -- rounding a0 to nearest would carry FLT_MAX to inf.  x == a0 + a1 + a2 exactly whenever x is a
//        multiple of bf16's smallest denormal 2^-133 -- every |x| >= 2^-110; below that the tail under 2^-133 is dropped.
//      * inf / NaN go into a0 alone (a NaN keeps a quiet bit, whatever its payload), a1 = a2 = 0: inf - inf is never formed.
//      * Layout = the product kernel's fragment order, zero-padded to whole tiles: a UNIT is 64 lanes x 16 bytes = the eight
//        consecutive-k bf16 values (k = 8 (lane / 32) .. + 7 of a 16-deep MFMA step) of the 32 rows lane % 32 of a block -- one
//        MFMA operand of a wave, 1 KiB.  Units are ordered [row tile][k-tile][plane][MFMA step][32-row block], so ALL the planes
//        of one k-tile of one row tile are one contiguous run (A: 24 KiB, B: 12 KiB).
//      * Scratch: 6 bytes an element of A padded to 256 x 16 and of B padded to 16 x 128.  Above SPLIT_SCRATCH_CAP = 1 GiB the
//        family does not apply (8192^3 takes 0.75 GiB) and today's routes run.
//  2. gemm_split_kernel<P>, P = 6 or 9 products: one workgroup of four waves (2 x 2) a 256 x 128 tile of C, a wave 128 x 64 = 4 x 2
//     blocks of 32 x 32 = 128 accumulator registers.
//      * K loop: k-tiles of 16 (one MFMA step), two LDS stages.  A k-tile's run goes global -> LDS as a STRAIGHT COPY by the
//        LDS DMA (__builtin_amdgcn_global_load_lds, 16 bytes a lane, 1 KiB = one unit a wave instruction; 36 a k-tile, 9 a wave):
//        no bounds checks (the planes are padded), one operand layout.  The DMA of k-tile t + 1 is issued ahead of the MFMAs
//        of k-tile t; the one barrier a k-tile retires it (the compiler's vmcnt(0) in front of s_barrier) and releases the stage
//        every wave has finished reading.  A fragment read is one ds_read_b128 at unit + 16 lane: consecutive lanes, consecutive
//        16 bytes, no bank conflict.
//      * LDS: a stage is (24 + 12) KiB = 36 KiB, two are 72 KiB: TWO workgroups a CU (144 of 160 KiB) = 2 waves a SIMD, each
//        with at most 256 registers (__launch_bounds__(256, 2)).  (A k-tile of 32 would be 144 KiB a workgroup, one wave a SIMD.)
//      * Per MFMA step a wave reads 3 x (4 + 2) fragments and issues 8 P MFMAs into ONE accumulator set, in a fixed order, low-order
//        products first: (a2 b2, a2 b1, a1 b2,) a2 b0, a0 b2, a1 b1, a1 b0, a0 b1, a0 b0.  That is the order of the products INTO EACH
//        accumulator (a data dependence the compiler keeps); across the eight blocks the compiler interleaves them as the fragments
//        arrive.  In the generated code the last fragment read, and with it the vmcnt(0) + barrier, sit about a third of the way
//        into a k-tile's MFMAs: the DMA of k-tile t + 1 overlaps only that third -- one reason the kernel is far from the ceiling.
//      * No atomics, no split of K: a repeated call gives the same bits.
//      * Epilogue where the sum is complete: alpha, beta Cin (apart from or aliasing C: an element is read and written by one
//        thread), the per-column bias, logistic / tanh (devmath.hpp); stores guarded for ragged M and N.
// Non-finite contract: an output element whose exact value is non-finite because of an inf / NaN operand element comes out
// non-finite -- possibly NaN where the fp32 chain gives +-inf (inf x a zero low piece).  Finite operands whose exact result is
// finite never produce a non-finite: no piece exceeds its x, and the pieces of one product are added smallest first.
// Plain HIP and builtins: the compiler places every wait.
#include "common.hpp"
#include "devmath.hpp"

namespace to {

constexpr int SP_TM = 256, SP_TN = 128, SP_KT = 16;        // the tile of C, the k-tile
constexpr int SP_WM = 2, SP_WN = 2;                        // waves along M / N
constexpr int SP_MI = SP_TM / 32 / SP_WM, SP_NJ = SP_TN / 32 / SP_WN;   // 32 x 32 blocks a wave
constexpr int SP_KS = SP_KT / 16;                          // MFMA steps a k-tile
constexpr int SP_A_UNITS = 3 * SP_KS * (SP_TM / 32), SP_B_UNITS = 3 * SP_KS * (SP_TN / 32);   // 1 KiB units a k-tile run
constexpr int SP_STAGE = (SP_A_UNITS + SP_B_UNITS) * 1024;
constexpr long long SPLIT_SCRATCH_CAP = 1LL << 30;
static_assert((SP_A_UNITS + SP_B_UNITS) % (SP_WM * SP_WN) == 0, "every wave issues the same number of DMA instructions");
static_assert(2 * 2 * SP_STAGE <= 160 * 1024, "two workgroups a CU");

// x = p[0] + p[1] + p[2], bf16 bit patterns, by truncation (the header)
__device__ __forceinline__ void split3(float x, unsigned (&p)[3]) {
  const unsigned u = __float_as_uint(x);
  if ((u & 0x7f800000u) == 0x7f800000u) {
    p[0] = (u >> 16) | ((u & 0x007fffffu) ? 0x0040u : 0u);
    p[1] = p[2] = 0u;
    return;
  }
  const unsigned h0 = u & 0xffff0000u;
  const float r1 = x - __uint_as_float(h0);
  const unsigned h1 = __float_as_uint(r1) & 0xffff0000u;
  const float r2 = r1 - __uint_as_float(h1);
  p[0] = h0 >> 16;
  p[1] = h1 >> 16;
  p[2] = __float_as_uint(r2) >> 16;
}

struct SplitOperand {
  const float* x;   // x[row * sx + k * sk]: rows are m (A) or n (B)
  uint4* planes;    // 3 * units units of 16 bytes
  long X, sx, sk;
  long units;       // padded rows x padded K / 8: the units of ONE plane
  int blocks;       // 32-row blocks a tile: SP_TM / 32 (A), SP_TN / 32 (B)
};
struct SplitPreArgs {
  SplitOperand o[2];
  long K;
  int nkt;
};

// one thread a unit lane: 8 consecutive k of one row, read guarded (zero outside), written to the three planes
__global__ __launch_bounds__(256) void gemm_split_pre_kernel(SplitPreArgs g) {
  const SplitOperand& o = g.o[blockIdx.y];
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= o.units) return;
  const int lane = (int)(t & 63);
  long q = t >> 6;
  const int xb = (int)(q % o.blocks);
  q /= o.blocks;
  const int ks = (int)(q % SP_KS);
  q /= SP_KS;                               // (row tile) * nkt + k-tile
  const long kt = q % g.nkt, xt = q / g.nkt;
  const long x = (xt * o.blocks + xb) * 32 + (lane & 31);
  const long k0 = (kt * SP_KS + ks) * 16 + (lane >> 5) * 8;
  unsigned w[3][4];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const long k = k0 + e;
    const float v = (x < o.X && k < g.K) ? o.x[x * o.sx + k * o.sk] : 0.0f;
    unsigned p[3];
    split3(v, p);
#pragma unroll
    for (int c = 0; c < 3; ++c) w[c][e / 2] = (e & 1) ? (w[c][e / 2] | (p[c] << 16)) : p[c];
  }
#pragma unroll
  for (int c = 0; c < 3; ++c)
    o.planes[((((q * 3 + c) * SP_KS + ks) * o.blocks + xb) << 6) + lane] = uint4{w[c][0], w[c][1], w[c][2], w[c][3]};
}

struct SplitArgs {
  const char* pa;   // the planes of A, of B (fragment order)
  const char* pb;
  float* C;
  const float* Cin;
  const float* bias;
  long M, N, c_sm;
  int nkt, tiles_n;
  float alpha, beta;
  int act;
};

typedef __bf16 sp_bf8 __attribute__((ext_vector_type(8)));
typedef float sp_f16 __attribute__((ext_vector_type(16)));

template <int P>
__global__ __launch_bounds__(256, 2) void gemm_split_kernel(SplitArgs g) {
  static_assert(P == 6 || P == 9, "six or nine products");
  typedef __attribute__((address_space(1))) const void* gptr_t;
  typedef __attribute__((address_space(3))) void* lptr_t;
  extern __shared__ __attribute__((aligned(1024))) char sp_lds[];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wm = wave / SP_WN, wn = wave % SP_WN;
  const long mt = blockIdx.x / g.tiles_n, nt = blockIdx.x % g.tiles_n;
  const char* arun = g.pa + mt * g.nkt * (long)(SP_A_UNITS * 1024) + lane * 16;
  const char* brun = g.pb + nt * g.nkt * (long)(SP_B_UNITS * 1024) + lane * 16;

  // k-tile t -> stage t & 1: unit u of the stage is unit u of A's run, or unit u - SP_A_UNITS of B's (the hardware adds 16 lane)
  auto issue = [&](int t) {
    char* st = sp_lds + (t & 1) * SP_STAGE;
    const char* a = arun + (long)t * (SP_A_UNITS * 1024);
    const char* b = brun + (long)t * (SP_B_UNITS * 1024);
#pragma unroll
    for (int q = 0; q < (SP_A_UNITS + SP_B_UNITS) / (SP_WM * SP_WN); ++q) {
      const int u = q * (SP_WM * SP_WN) + wave;
      const char* src = u < SP_A_UNITS ? a + u * 1024 : b + (u - SP_A_UNITS) * 1024;
      __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(st + u * 1024), 16, 0, 0);
    }
  };

  sp_f16 acc[SP_MI][SP_NJ];
#pragma unroll
  for (int i = 0; i < SP_MI; ++i)
#pragma unroll
    for (int j = 0; j < SP_NJ; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

  // (piece of A, piece of B), low-order products first; six products start at entry 3
  constexpr int ORD[9][2] = {{2, 2}, {2, 1}, {1, 2}, {2, 0}, {0, 2}, {1, 1}, {1, 0}, {0, 1}, {0, 0}};

  issue(0);
  __syncthreads();
  for (int t = 0; t < g.nkt; ++t) {
    if (t + 1 < g.nkt) issue(t + 1);
    const char* st = sp_lds + (t & 1) * SP_STAGE + lane * 16;
#pragma unroll
    for (int ks = 0; ks < SP_KS; ++ks) {
      sp_bf8 a[3][SP_MI], b[3][SP_NJ];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
#pragma unroll
        for (int i = 0; i < SP_MI; ++i)
          a[c][i] = *reinterpret_cast<const sp_bf8*>(st + ((c * SP_KS + ks) * (SP_TM / 32) + wm * SP_MI + i) * 1024);
#pragma unroll
        for (int j = 0; j < SP_NJ; ++j)
          b[c][j] = *reinterpret_cast<const sp_bf8*>(st + (SP_A_UNITS + (c * SP_KS + ks) * (SP_TN / 32) + wn * SP_NJ + j) * 1024);
      }
#pragma unroll
      for (int o = 9 - P; o < 9; ++o)
#pragma unroll
        for (int i = 0; i < SP_MI; ++i)
#pragma unroll
          for (int j = 0; j < SP_NJ; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[ORD[o][0]][i], b[ORD[o][1]][j], acc[i][j], 0, 0, 0);
    }
    __syncthreads();   // retires the DMA of k-tile t + 1; every wave has read stage t & 1
  }

  // accumulator register r of a block: row 8 (r / 4) + 4 (lane / 32) + r % 4, column lane % 32
#pragma unroll
  for (int i = 0; i < SP_MI; ++i)
#pragma unroll
    for (int j = 0; j < SP_NJ; ++j) {
      const long n = nt * SP_TN + (wn * SP_NJ + j) * 32 + (lane & 31);
      if (n >= g.N) continue;
      const float bias = g.bias ? g.bias[n] : 0.0f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const long m = mt * SP_TM + (wm * SP_MI + i) * 32 + 8 * (r / 4) + 4 * (lane >> 5) + (r & 3);
        if (m >= g.M) continue;
        float v = g.alpha * acc[i][j][r];
        if (g.beta != 0.0f) v += g.beta * g.Cin[m * g.c_sm + n];
        if (g.bias) v += bias;
        if (g.act == 1) v = dm::logistic(v);
        else if (g.act == 2) v = dm::tanh(v);
        g.C[m * g.c_sm + n] = v;
      }
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------

// to_set_gemm_f32_split: 0 off (default), 1 the scanned rows below, 2 wherever split_pick holds; products 6 or 9
static int g_split_mode = 0, g_split_products = 6;

bool gemm_split_set(int mode, int products, int* previous_mode) {
  if (mode < 0 || mode > 2 || (products != -1 && products != 6 && products != 9)) return false;
  if (previous_mode) *previous_mode = g_split_mode;
  g_split_mode = mode;
  g_split_products = products == -1 ? 6 : products;
  return true;
}

static long long split_scratch_bytes(const GemmProblem& p) {
  const long long mp = (p.M + SP_TM - 1) / SP_TM * SP_TM, np = (p.N + SP_TN - 1) / SP_TN * SP_TN, kp = (p.K + SP_KT - 1) / SP_KT * SP_KT;
  return 6 * (mp + np) * kp;
}

// In scope?  (What the plan's gemv question takes first -- M or N = 1 streams, K = 1 outer products, K < 16 updates of large C -- is
// refused here, so that both planner predicates see what the plan does; the few-rhs and skinny-K families are asked first too.)
static bool split_pick(const GemmProblem& p) {
  if (p.dtype != TO_F32 || p.batch != 1 || p.reduce_batch || p.rowsum || p.loss_rows || p.dact || p.tail_out || p.a_table ||
      p.M < 1 || p.N < 1 || p.K < 1 || (p.beta != 0.0 && !p.Cin) || p.act < 0 || p.act > 2)
    return false;
  if (p.M > 2147483647LL - SP_TM || p.N > 2147483647LL - SP_TN || p.K > 2147483647LL - SP_KT) return false;
  if (p.a_sm < 0 || p.a_sk < 0 || p.b_sk < 0 || p.b_sn < 0 || p.c_sm < 0) return false;
  if (((p.M + SP_TM - 1) / SP_TM) * ((p.N + SP_TN - 1) / SP_TN) > 2147483647LL) return false;
  if (split_scratch_bytes(p) > SPLIT_SCRATCH_CAP) return false;
  return !gemv_form(p, true);
}

// Mode 1: the rows of tools/gemm_split_scan.py (profiles/gemm_split_scan.txt) where mode 2 measured ahead of today's route by more
// than twice the row's larger spread (0.003), per product count; everything unscanned keeps its route -- a scanned row is the
// plain product (alpha 1, no beta Cin / bias / activation) of row-major A and B, and gemm_plan asks for top-level problems only
// (a 4096^3 block of a larger, unscanned product keeps its route; mode 1 changes no planner predicate).  us today -> six / nine
// products, pre-pass included: 4096^3 916 -> 705 / 925 (nine is behind: not taken), 8192^3 7283 -> 5292 / 7001.  Behind today's
// route and left alone: 1024^3 (0.18), 2048^3 (0.65), 1088^3 (0.26), 1472^3 (0.42), 1280 x 4096 x 1280 (0.31), 60000 x 784 x 300
// (0.53), 60000 x 300 x 100 (0.28).
struct SplitScanned { int m, k, n; bool six, nine; };
static const SplitScanned split_scanned[] = {
    {4096, 4096, 4096, true, false},
    {8192, 8192, 8192, true, true},
};
static bool split_auto(const GemmProblem& p) {
  if (p.a_sk != 1 || p.b_sn != 1 || p.alpha != 1.0 || p.beta != 0.0 || p.bias || p.act) return false;   // (as scanned)
  for (const SplitScanned& r : split_scanned)
    if (r.m == p.M && r.k == p.K && r.n == p.N) return g_split_products == 9 ? r.nine : r.six;
  return false;
}

bool gemm_split_applicable(const GemmProblem& p) {
  if (g_split_mode == 0 || !split_pick(p)) return false;
  return g_split_mode == 2 || split_auto(p);
}

bool gemm_split_everywhere(const GemmProblem& p) { return g_split_mode == 2 && split_pick(p); }

void launch_gemm_split(const GemmProblem& p, hipStream_t s) {
  TO_CHECK(split_pick(p), TO_ERR_STATE, "launch_gemm_split: not applicable");
  const long mt = (p.M + SP_TM - 1) / SP_TM, nt = (p.N + SP_TN - 1) / SP_TN, nkt = (p.K + SP_KT - 1) / SP_KT;
  const long ua = mt * SP_TM * nkt * SP_KT / 8, ub = nt * SP_TN * nkt * SP_KT / 8;   // 16-byte units of one plane
  const int64_t sd[2] = {1, (int64_t)(3 * (ua + ub) * 4)};                           // ... as floats
  Holder scratch(new_tensor(2, sd, 0, TO_F32));
  uint4* planes = static_cast<uint4*>(scratch.t->ptr);

  SplitPreArgs pre{};
  pre.o[0] = SplitOperand{static_cast<const float*>(p.A), planes, p.M, p.a_sm, p.a_sk, ua, SP_TM / 32};
  pre.o[1] = SplitOperand{static_cast<const float*>(p.B), planes + 3 * ua, p.N, p.b_sn, p.b_sk, ub, SP_TN / 32};
  pre.K = p.K;
  pre.nkt = (int)nkt;
  const long umax = ua > ub ? ua : ub;
  launch_k(gemm_split_pre_kernel, dim3((unsigned)((umax + 255) / 256), 2), dim3(256), 0, s, pre);
  TO_HIP(hipGetLastError());
  count_launch();

  SplitArgs g{};
  g.pa = reinterpret_cast<const char*>(planes);
  g.pb = reinterpret_cast<const char*>(planes + 3 * ua);
  g.C = static_cast<float*>(p.C);
  g.Cin = static_cast<const float*>(p.Cin);
  g.bias = static_cast<const float*>(p.bias);
  g.M = p.M; g.N = p.N; g.c_sm = p.c_sm;
  g.nkt = (int)nkt; g.tiles_n = (int)nt;
  g.alpha = (float)p.alpha; g.beta = (float)p.beta; g.act = p.act;
  static bool attr_set[2] = {false, false};
  auto go = [&](auto kern, int which) {
    if (!attr_set[which]) {
      TO_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 2 * SP_STAGE));
      attr_set[which] = true;
    }
    launch_k(kern, dim3((unsigned)(mt * nt)), dim3(256), 2 * SP_STAGE, s, g);
  };
  if (g_split_products == 9) go(gemm_split_kernel<9>, 1);
  else go(gemm_split_kernel<6>, 0);
  TO_HIP(hipGetLastError());
  count_launch();
}

}  // namespace to
