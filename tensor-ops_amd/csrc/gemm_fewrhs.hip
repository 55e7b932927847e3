// A few right-hand sides beside a long extent: C[M x N] = alpha A[M x K] B[K x N] (+ beta Cin) (+ bias) (activation) with
// 2 <= N <= 32 (A is streamed) or 2 <= M <= 32 (B is streamed: the same kernel on strides, C^T = B^T A^T), batch 1, fp32 / fp64.
// Off unless to_set_gemm_few_rhs turns it on.
//
// Such a product moves every element of the big operand once and does at most 32 multiply-adds on it: the bound is HBM, and the
// design is gemv.hip's widened to a handful of right-hand sides on 16x16x4 MFMA blocks.  Names: L the long extent, F the narrow
// one (padded to FP = 16 or 32: one or two column blocks), S[l][k] the streamed operand, W[k][f] the narrow one.
//
//  * K runs in groups of G = 4 V elements, V = 4 (fp32) or 2 (fp64) the elements of 16 bytes.  MFMA step e < V of a group takes
//    k = group + V kg + e from the lanes of k-group kg = lane / 16: both storage orders below use this one permutation of k,
//    so one image of W serves both.
//  * W lives in LDS, zero-padded to FP columns and to whole groups, at ((k / V) FP + f) V + k % V: the V values a lane needs
//    for the V steps of a group are ONE 16-byte LDS read per column block.  It is taken in chunks of FEWRHS_CHUNK_BYTES =
//    16 KiB -- 16 KiB / (FP x element size) values of k: 256 / 128 (fp32, 16 / 32 columns), 128 / 64 (fp64) -- shared by the
//    workgroup's four waves and DOUBLE-BUFFERED: the next chunk is loaded into registers ahead of the current chunk's MFMAs
//    and written to the other buffer behind them, so ONE barrier a chunk change is enough (a wave that overwrites a buffer
//    has passed the barrier every reader of that buffer's previous chunk arrived at after its last read).  The issue's 64 KiB
//    chunk would have left one workgroup (four waves) a CU; 2 x 16 KiB leave five, the ~16 waves a CU the stream needs.
//  * S goes from global memory straight into the MFMA fragment, 16 bytes a lane, four loads in flight a wave, no LDS trip:
//      - k-contiguous rows (LC = false): a wave owns 16 rows; a lane's 16 bytes are k = group + V kg .. + V - 1 of row
//        lane % 16 and feed the A slot of the group's V MFMAs; W's 16 bytes feed the B slot.
//      - long-axis-contiguous storage (LC = true): a wave owns 16 V rows; a lane's 16 bytes are rows V (lane % 16) .. + V - 1
//        at one k, V loads a group; they feed the B slot (one accumulator per row residue e), W feeds the A slot, and the
//        tile comes out transposed: output row V (lane % 16) + e, column 4 kg + r (fp64: kg + 4 r, its accumulator layout).
//    Where the base or the stride between 16-byte pieces is not 16-byte aligned (VEC = false) the same lane loads the same
//    elements one by one, so the bits do not depend on alignment.  The K tail (the last, partial group), a split's end and a
//    ragged last row block take guarded element loads in the same launch; the padding is SELECTED zero, never multiplied.
//  * Too few row blocks for ~256 x 16 waves under a long K: K is split over blockIdx.y (at most 256 parts, whole groups
//    each), partial sums go to a [splits][L][F] pool workspace, and gemm_fewrhs_finish_kernel adds them in split order and
//    applies the epilogue -- no atomics, the same bits every run (gemv_finish_kernel's contract).
//  * alpha, beta Cin (apart from or aliasing C: an element is read and written by one thread), the per-column bias and
//    logistic / tanh are applied where the sum is complete.
// Plain HIP and builtins: the compiler places every wait.
#include "common.hpp"
#include "devmath.hpp"

namespace to {

constexpr int FEWRHS_CHUNK_BYTES = 16384;

template <class S> struct FewT;
template <> struct FewT<float> {
  typedef float vec __attribute__((ext_vector_type(4)));
  typedef float acc __attribute__((ext_vector_type(4)));
};
template <> struct FewT<double> {
  typedef double vec __attribute__((ext_vector_type(2)));
  typedef double acc __attribute__((ext_vector_type(4)));
};
__device__ __forceinline__ FewT<float>::acc few_mfma(float a, float b, FewT<float>::acc c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ FewT<double>::acc few_mfma(double a, double b, FewT<double>::acc c) {
  return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}

struct FewArgs {
  const void* S;        // streamed: S[l * s_sl + k * s_sk], one of the two strides is 1
  const void* W;        // narrow:   W[k * w_sk + f * w_sf]
  void* C;              // C[l * c_sl + f * c_sf]
  const void* Cin;      // laid out as C
  const void* bias;     // per column of the PRODUCT: bias[f], or bias[l] where the narrow extent is M
  void* part;           // [gridDim.y][L][F] when K is split
  long L, K, s_sl, s_sk, w_sk, w_sf, c_sl, c_sf;
  long k_per;           // k per split, a multiple of G
  double alpha, beta;
  int F, act, bias_on_long;
};

template <class S>
__device__ __forceinline__ S few_epilogue(const FewArgs& g, S acc, long l, int f) {
  S v = (S)g.alpha * acc;
  if (g.beta != 0.0) v += (S)g.beta * static_cast<const S*>(g.Cin)[l * g.c_sl + f * g.c_sf];
  if (g.bias) v += static_cast<const S*>(g.bias)[g.bias_on_long ? l : (long)f];
  if (g.act == 1) v = dm::logistic(v);
  else if (g.act == 2) v = tanh(v);
  return v;
}

// CB: column blocks (F <= 16 CB); LC: S is contiguous along the long axis; VEC: 16-byte loads of S
template <class S, int CB, bool LC, bool VEC>
__global__ __launch_bounds__(256) void gemm_fewrhs_kernel(FewArgs g) {
  typedef typename FewT<S>::vec SV;
  typedef typename FewT<S>::acc SA;
  constexpr int V = 16 / (int)sizeof(S), G = 4 * V, FP = 16 * CB, KC = FEWRHS_CHUNK_BYTES / (FP * (int)sizeof(S));
  constexpr int NE = LC ? V : 1, RB = 16 * NE;    // accumulators a column block; rows a wave
  constexpr int NL = LC ? V : 1;                  // 16-byte loads a group
  constexpr int UN = 4 / NL;                      // groups a trip of the unrolled loop: four loads in flight
  constexpr int EPT = KC * FP / 256;              // elements of a chunk a thread stages
  static_assert(KC % (UN * G) == 0, "a chunk is whole trips");
  __shared__ __attribute__((aligned(16))) S wl[2][KC * FP];
  const S* __restrict__ Sm = static_cast<const S*>(g.S);
  const S* __restrict__ Wm = static_cast<const S*>(g.W);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, kg = lane >> 4;
  const long l0 = ((long)blockIdx.x * 4 + wave) * RB;
  const long k0 = (long)blockIdx.y * g.k_per, k1 = k0 + g.k_per < g.K ? k0 + g.k_per : g.K;
  const bool live = l0 < g.L, rows_full = l0 + RB <= g.L;
  const bool f_fast = g.w_sf == 1;   // W's columns are contiguous: neighbouring threads take neighbouring columns (else neighbouring k)

  // a chunk of W: global -> registers (zeros selected beyond the split's end and beyond F) ...
  auto w_load = [&](long kc, S (&r)[EPT]) {
#pragma unroll
    for (int i = 0; i < EPT; ++i) {
      const int e = threadIdx.x + 256 * i;
      const int j = f_fast ? e & (FP - 1) : e / KC, kk = f_fast ? e / FP : e & (KC - 1);
      const long k = kc + kk;
      r[i] = (k < k1 && j < g.F) ? Wm[k * g.w_sk + j * g.w_sf] : S(0);
    }
  };
  // ... -> LDS, the whole groups the chunk has
  auto w_store = [&](int buf, long kc, const S (&r)[EPT]) {
    const long left = (k1 - kc + G - 1) / G * G;
    const int kn = left < KC ? (int)left : KC;
#pragma unroll
    for (int i = 0; i < EPT; ++i) {
      const int e = threadIdx.x + 256 * i;
      const int j = f_fast ? e & (FP - 1) : e / KC, kk = f_fast ? e / FP : e & (KC - 1);
      if (kk < kn) wl[buf][((kk / V) * FP + j) * V + (kk % V)] = r[i];
    }
  };

  struct Frag { SV s[NL]; };
  const long lrow = l0 + c < g.L ? l0 + c : g.L - 1;   // (LC = false: rows past the end load the last row; never stored)
  const S* __restrict__ sp = LC ? Sm + (l0 + V * c) + (long)(V * kg) * g.s_sk : Sm + lrow * g.s_sl + V * kg;
  // the group at kb: unguarded where the group and the wave's rows are whole, guarded element loads elsewhere
  auto s_load = [&](long kb, Frag& f, bool whole) {
    if (whole) {
#pragma unroll
      for (int u = 0; u < NL; ++u) {
        const S* q = LC ? sp + (kb + u) * g.s_sk : sp + kb;
        if constexpr (VEC) {
          f.s[u] = *reinterpret_cast<const SV*>(q);
        } else {
#pragma unroll
          for (int e = 0; e < V; ++e) f.s[u][e] = q[e];
        }
      }
    } else {
#pragma unroll
      for (int u = 0; u < NL; ++u)
#pragma unroll
        for (int e = 0; e < V; ++e) {
          const long k = kb + V * kg + (LC ? u : e);
          const bool in = k < k1 && (!LC || l0 + V * c + e < g.L);
          const S* q = LC ? sp + (kb + u) * g.s_sk + e : sp + kb + e;
          f.s[u][e] = in ? *q : S(0);
        }
    }
  };

  SA acc[NE][CB];
#pragma unroll
  for (int e = 0; e < NE; ++e)
#pragma unroll
    for (int b = 0; b < CB; ++b) acc[e][b] = SA{S(0), S(0), S(0), S(0)};
  // the group whose first k sits `off` into the chunk in wb
  auto mac = [&](const S* wb, int off, const Frag& f) {
#pragma unroll
    for (int b = 0; b < CB; ++b) {
      const SV w = *reinterpret_cast<const SV*>(wb + ((off / V + kg) * FP + 16 * b + c) * V);
      if constexpr (LC) {
#pragma unroll
        for (int u = 0; u < V; ++u)
#pragma unroll
          for (int e = 0; e < V; ++e) acc[e][b] = few_mfma(w[u], f.s[u][e], acc[e][b]);
      } else {
#pragma unroll
        for (int e = 0; e < V; ++e) acc[0][b] = few_mfma(f.s[0][e], w[e], acc[0][b]);
      }
    }
  };

  S wr[EPT];
  w_load(k0, wr);
  w_store(0, k0, wr);
  __syncthreads();
  int buf = 0;
  for (long kc = k0; kc < k1; kc += KC, buf ^= 1) {
    const bool more = kc + KC < k1;
    if (more) w_load(kc + KC, wr);
    if (live) {
      const long kend = kc + KC < k1 ? kc + KC : k1;
      const S* wb = wl[buf];
      long kb = kc;
      if (!LC || rows_full) {
        for (; kb + UN * G <= kend; kb += UN * G) {
          Frag f[UN];
#pragma unroll
          for (int t = 0; t < UN; ++t) s_load(kb + t * G, f[t], true);
#pragma unroll
          for (int t = 0; t < UN; ++t) mac(wb, (int)(kb - kc) + t * G, f[t]);
        }
      }
      for (; kb < kend; kb += G) {
        Frag f;
        s_load(kb, f, kb + G <= kend && (!LC || rows_full));
        mac(wb, (int)(kb - kc), f);
      }
    }
    if (more) {
      w_store(buf ^ 1, kc + KC, wr);
      __syncthreads();
    }
  }
  if (!live) return;

  auto put = [&](long l, int f, S a) {
    if (l >= g.L || f >= g.F) return;
    if (gridDim.y > 1) static_cast<S*>(g.part)[((long)blockIdx.y * g.L + l) * g.F + f] = a;
    else static_cast<S*>(g.C)[l * g.c_sl + f * g.c_sf] = few_epilogue<S>(g, a, l, f);
  };
#pragma unroll
  for (int e = 0; e < NE; ++e)
#pragma unroll
    for (int b = 0; b < CB; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = sizeof(S) == 8 ? kg + 4 * r : 4 * kg + r;   // the block's row in accumulator register r (fp64 / fp32 layout)
        if constexpr (LC) put(l0 + V * c + e, 16 * b + i, acc[e][b][r]);   // (the tile is C^T: rows of the block are f)
        else put(l0 + i, 16 * b + c, acc[0][b][r]);
      }
}

// C[l][f] = epilogue(sum over the splits, in split order)
template <class S>
__global__ __launch_bounds__(256) void gemm_fewrhs_finish_kernel(FewArgs g, int splits) {
  const long o = (long)blockIdx.x * 256 + threadIdx.x, LF = g.L * g.F;
  if (o >= LF) return;
  const S* part = static_cast<const S*>(g.part);
  S acc = S(0);
  int sp = 0;
  for (; sp + 8 <= splits; sp += 8) {   // (eight loads in flight; the order of the additions is fixed)
    S t[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) t[e] = part[(long)(sp + e) * LF + o];
#pragma unroll
    for (int e = 0; e < 8; ++e) acc += t[e];
  }
  for (; sp < splits; ++sp) acc += part[(long)sp * LF + o];
  const long l = o / g.F;
  const int f = (int)(o - l * g.F);
  static_cast<S*>(g.C)[l * g.c_sl + f * g.c_sf] = few_epilogue<S>(g, acc, l, f);
}

// ---- host side ---------------------------------------------------------------------------------------------------------------

// to_set_gemm_few_rhs: 0 off (default), 1 the scanned shape classes below, 2 wherever fewrhs_pick holds; splits -1 / 1 .. 256
static int g_fewrhs_mode = 0, g_fewrhs_splits = -1;

bool gemm_fewrhs_set(int mode, int splits, int* previous_mode) {
  if (mode < 0 || mode > 2 || splits == 0 || splits < -1 || splits > 256) return false;
  if (previous_mode) *previous_mode = g_fewrhs_mode;
  g_fewrhs_mode = mode;
  g_fewrhs_splits = splits;
  return true;
}

// In range?  *stream_b: the narrow extent is M and B is streamed.  Both narrow: the larger operand is streamed (A at a tie);
// if that one is contiguous along neither axis, the other one.
static bool fewrhs_pick(const GemmProblem& p, bool* stream_b) {
  if ((p.dtype != TO_F32 && p.dtype != TO_F64) || p.batch != 1 || p.reduce_batch || p.rowsum || p.loss_rows || p.dact || p.tail_out ||
      p.a_table || p.M < 1 || p.N < 1 || p.K < 1 || (p.beta != 0.0 && !p.Cin) || p.act < 0 || p.act > 2)
    return false;
  if (p.M > 2147483647LL || p.N > 2147483647LL || p.K > 2147483647LL) return false;
  if (p.a_sm < 0 || p.a_sk < 0 || p.b_sk < 0 || p.b_sn < 0 || p.c_sm < 0) return false;
  const bool a_ok = p.N >= 2 && p.N <= 32 && (p.a_sk == 1 || p.a_sm == 1);   // stream A
  const bool b_ok = p.M >= 2 && p.M <= 32 && (p.b_sk == 1 || p.b_sn == 1);   // stream B
  if (!a_ok && !b_ok) return false;
  *stream_b = a_ok && b_ok ? p.N > p.M : b_ok;
  return true;
}

// Mode 1: the shape classes tools/gemm_fewrhs_scan.py measured ahead of today's route by more than the run-to-run spread it
// prints (profiles/gemm_fewrhs_scan.txt); everything unscanned keeps its route.  The bar is today / fewrhs above 1 + twice the
// row's spread (0.001 .. 0.013) in every storage order scanned.  us today -> here: fp32 60000 x 100 x 10 22.5 -> 10.7, 60000 x 784
// x 10 98.3 -> 44.2 (A stored transposed: 91.6 -> 78.5); fp64 60000 x 100 x 10 60.4 -> 10.6, 60000 x 784 x 10 403.2 -> 75.5
// (transposed 387.7 -> 67.9), 60000 x 300 x 32 52.5 -> 32.3, 1024 x 60000 x 32 773.8 -> 114.0, 10 x 60000 x 100 290.8 -> 40.6.
// Behind today's route and left alone: fp32 60000 x 300 x 32 (0.83), 1024 x 60000 x 32 (0.85), 10 x 60000 x 100 (0.91), 60000 x
// 10000 x 8 (0.94), 10000 x 60000 x 32 (0.85), 32 x 10000 x 60000 (0.44) and 8 x 60000 x 10000 (0.50; 1.09 with B stored transposed).
struct FewScanned { int dtype; int m, k, n; };
static const FewScanned fewrhs_scanned[] = {
    {TO_F32, 60000, 100, 10}, {TO_F32, 60000, 784, 10},
    {TO_F64, 60000, 100, 10}, {TO_F64, 60000, 784, 10}, {TO_F64, 60000, 300, 32}, {TO_F64, 1024, 60000, 32}, {TO_F64, 10, 60000, 100},
};
static bool fewrhs_auto(const GemmProblem& p) {
  for (const FewScanned& r : fewrhs_scanned)
    if (r.dtype == p.dtype && r.m == p.M && r.k == p.K && r.n == p.N) return true;
  return false;
}

bool gemm_fewrhs_applicable(const GemmProblem& p) {
  bool sb;
  if (g_fewrhs_mode == 0 || !fewrhs_pick(p, &sb)) return false;
  return g_fewrhs_mode == 2 || fewrhs_auto(p);
}

bool gemm_fewrhs_everywhere(const GemmProblem& p) {
  bool sb;
  return g_fewrhs_mode == 2 && fewrhs_pick(p, &sb);
}

template <class S>
static void fewrhs_launch(FewArgs g, hipStream_t s) {
  constexpr int V = 16 / (int)sizeof(S), G = 4 * V;
  const int dtype = sizeof(S) == 8 ? TO_F64 : TO_F32;
  const bool lc = g.s_sk != 1;   // (fewrhs_pick: then s_sl == 1)
  const bool vec = (reinterpret_cast<uintptr_t>(g.S) & 15u) == 0 && (lc ? g.s_sk : g.s_sl) % V == 0;
  const long rb = lc ? 16 * V : 16, waves = (g.L + rb - 1) / rb;
  const long target_waves = 256L * 16;   // enough waves in flight to cover the HBM latency
  long splits = 1;
  if (g_fewrhs_splits > 0) {
    splits = g_fewrhs_splits;
  } else if (waves < target_waves && g.K >= 2048) {   // (at least 512 k a part: a part pays for its own image of W and its partial store)
    splits = (target_waves + waves - 1) / waves;
    if (splits > g.K / 512) splits = g.K / 512;
    if (splits > 256) splits = 256;
  }
  if (splits > g.K) splits = g.K;
  g.k_per = ((g.K + splits - 1) / splits + G - 1) / G * G;
  splits = (g.K + g.k_per - 1) / g.k_per;
  Holder tmp;
  if (splits > 1) {
    const int64_t pd[2] = {splits, g.L * g.F};
    tmp.t = new_tensor(2, pd, 0, dtype);
    g.part = tmp.t->ptr;
  }
  const dim3 grid((unsigned)((waves + 3) / 4), (unsigned)splits);
#define FEW_GO(CB) do { \
    if (lc) { if (vec) launch_k((gemm_fewrhs_kernel<S, CB, true, true>), grid, dim3(256), 0, s, g); \
              else launch_k((gemm_fewrhs_kernel<S, CB, true, false>), grid, dim3(256), 0, s, g); } \
    else { if (vec) launch_k((gemm_fewrhs_kernel<S, CB, false, true>), grid, dim3(256), 0, s, g); \
           else launch_k((gemm_fewrhs_kernel<S, CB, false, false>), grid, dim3(256), 0, s, g); } } while (0)
  if (g.F <= 16) FEW_GO(1);
  else FEW_GO(2);
#undef FEW_GO
  TO_HIP(hipGetLastError());
  count_launch();
  if (splits > 1) {
    launch_k((gemm_fewrhs_finish_kernel<S>), dim3((unsigned)((g.L * g.F + 255) / 256)), dim3(256), 0, s, g, (int)splits);
    TO_HIP(hipGetLastError());
    count_launch();
  }
}

void launch_gemm_fewrhs(const GemmProblem& p, hipStream_t s) {
  bool sb = false;
  TO_CHECK(fewrhs_pick(p, &sb), TO_ERR_STATE, "launch_gemm_fewrhs: not applicable");
  FewArgs g{};
  if (sb) {   // C^T = B^T A^T
    g.S = p.B; g.s_sl = p.b_sn; g.s_sk = p.b_sk; g.W = p.A; g.w_sk = p.a_sk; g.w_sf = p.a_sm;
    g.L = p.N; g.F = (int)p.M; g.c_sl = 1; g.c_sf = p.c_sm; g.bias_on_long = 1;
  } else {
    g.S = p.A; g.s_sl = p.a_sm; g.s_sk = p.a_sk; g.W = p.B; g.w_sk = p.b_sk; g.w_sf = p.b_sn;
    g.L = p.M; g.F = (int)p.N; g.c_sl = p.c_sm; g.c_sf = 1; g.bias_on_long = 0;
  }
  g.K = p.K; g.C = p.C; g.Cin = p.Cin; g.bias = p.bias;
  g.alpha = p.alpha; g.beta = p.beta; g.act = p.act;
  if (p.dtype == TO_F64) fewrhs_launch<double>(g, s);
  else fewrhs_launch<float>(g, s);
}

}  // namespace to
