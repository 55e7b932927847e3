// What to_rnn_stack_*_ragged (stack_rnn.cpp) adds to the dense entries: a batch whose sequences have different lengths.
// The sequences are sorted by length, descending and stable (perm: sorted position -> sequence), and their steps PACKED
// time-major: at step t the active sequences are the first cnt[t] sorted positions, and their rows are the contiguous
// packed rows off[t] .. off[t] + cnt[t] - 1 (off: the exclusive prefix sum of cnt; N = off[Tmax] = the sum of the
// lengths).  Everything that does not depend on time is then one contraction over exactly N rows, by the dense path's own
// calls; padding never enters one.  This file holds what is left:
//   pack     the caller's strided [B; T, n] -> packed [N][n]                       (padding is not read)
//   unpack   packed [N][n] -> the caller's contiguous [B; T, n], +0.0 at padding
//   rnn_ragged_seq_kernel   rnn_seq.hip's persistent recurrence on packed rows
//   shift / initial / final state movers of one launch each.
// The device tables (RaggedTables) are O(B + T) int32 and uploaded once a call; a packed row's (t, p) is found by a binary
// search over off.  A stateful layer keeps two arrays aligned row for row with Z: Sa(t, p) the state after step t, Sp(t, p)
// the state before it (block 0: the initial states).
#include <algorithm>
#include <cstdint>

#include "common.hpp"
#include "devmath.hpp"

namespace to {

namespace {

constexpr int RAG_THREADS = 256;
constexpr int RAG_QMAX = RNN_SEQ_MAX_H / RAG_THREADS;  // (row, column) items per thread, as rnn_seq.hip
constexpr size_t RAG_LDS_MAX = 160 * 1024;

struct alignas(16) Piece16 { unsigned v[4]; };

// the step of packed row r: the largest t < Tmax with off[t] <= r  (r < off[Tmax])
__device__ __forceinline__ int step_of(const int* __restrict__ off, int Tmax, long r) {
  int lo = 0, hi = Tmax - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if ((long)off[mid] <= r) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// dst[r][j] = src(perm[p], t, j), r = off[t] + p < N; a piece P is one element (feature stride sj, in pieces) or 16 bytes
// (sj = 1).  sb / st: bytes between sequences / steps of the source.
template <class P>
__global__ __launch_bounds__(RAG_THREADS) void ragged_pack_kernel(const char* __restrict__ src, P* __restrict__ dst,
                                                                  RaggedTables tb, long sb, long st, long sj, long npr) {
  const long total = (long)tb.N * npr, stride = (long)gridDim.x * RAG_THREADS;
  for (long e = (long)blockIdx.x * RAG_THREADS + threadIdx.x; e < total; e += stride) {
    const long r = e / npr, j = e - r * npr;
    const int t = step_of(tb.off, tb.Tmax, r);
    const long b = tb.perm[r - tb.off[t]];
    dst[e] = reinterpret_cast<const P*>(src + b * sb + (long)t * st)[j * sj];
  }
}

// dst [B][T][npr] contiguous: row (b, t) = packed row off[t] + inv[b] when t < lens[b], zero otherwise
template <class P>
__global__ __launch_bounds__(RAG_THREADS) void ragged_unpack_kernel(const P* __restrict__ src, P* __restrict__ dst,
                                                                    RaggedTables tb, long T, long npr) {
  const long total = (long)tb.B * T * npr, stride = (long)gridDim.x * RAG_THREADS;
  for (long e = (long)blockIdx.x * RAG_THREADS + threadIdx.x; e < total; e += stride) {
    const long row = e / npr, j = e - row * npr;
    const long b = row / T, t = row - b * T;
    P v{};
    if (t < (long)tb.lens[b]) v = src[((long)tb.off[t] + tb.inv[b]) * npr + j];
    dst[e] = v;
  }
}

// mode 0: Sp block 0 [B][n] = the batched initial states of the sorted sequences, dst[p][j] = src[perm[p] * sb + j * ss]
// mode 1: s_out [B][n] = the state after each sequence's last step,             dst[b][j] = Sa[off[lens[b]-1] + inv[b]][j]
// mode 2: Sp blocks 1.. from Sa (the per-step route),      dst[r][j] = Sa[off[t-1] + p][j], r = off[t] + p, B <= r < N
template <class S, int MODE>
__global__ __launch_bounds__(RAG_THREADS) void ragged_state_kernel(const S* __restrict__ src, S* __restrict__ dst,
                                                                   RaggedTables tb, long n, long sb, long ss) {
  const long first = MODE == 2 ? tb.B : 0, last = MODE == 2 ? tb.N : tb.B;
  const long total = (last - first) * n, stride = (long)gridDim.x * RAG_THREADS;
  for (long e = (long)blockIdx.x * RAG_THREADS + threadIdx.x; e < total; e += stride) {
    const long q = e / n, j = e - q * n, r = first + q;
    if constexpr (MODE == 0) {
      dst[r * n + j] = src[(long)tb.perm[r] * sb + j * ss];
    } else if constexpr (MODE == 1) {
      dst[r * n + j] = src[((long)tb.off[tb.lens[r] - 1] + tb.inv[r]) * n + j];
    } else {
      const int t = step_of(tb.off, tb.Tmax, r);
      dst[r * n + j] = src[((long)tb.off[t - 1] + (r - tb.off[t])) * n + j];
    }
  }
}

template <class S>
struct RaggedSeqArgs {
  const S* M;  // [H][H]: out[j] = sum_k v[k] M[k][j]
  S* Z;        // [N][H] packed: forward P -> z, reverse G -> dz, in place
  S* Sa;       // [N][H]: forward writes the state after each step; reverse reads it
  S* Sp;       // [N][H]: forward reads block 0 (the initial states) and writes the state before each later step
  int H, R;
};

// rnn_seq_kernel on packed rows.  A workgroup owns R consecutive SORTED positions and all H columns; its first row is its
// longest, so it loops to that row's length only -- every thread of it counts the same barriers -- and a workgroup of short
// sequences is done early.  Forward: a row drops out at t == its length and touches nothing after.  Reverse: a row joins at
// t == its length - 1 with an incoming dz of zero.  off[t] is uniform across the workgroup and read from the table each
// step (T is unbounded: no copy of it in LDS).
template <class S, bool REV, bool MLDS, int ACT>
__global__ __launch_bounds__(RAG_THREADS) void rnn_ragged_seq_kernel(RaggedSeqArgs<S> a, RaggedTables tb) {
  extern __shared__ __align__(16) unsigned char rag_lds[];
  const int H = a.H, R = a.R;
  S* v = reinterpret_cast<S*>(rag_lds);  // [2][R][H]
  S* Ml = v + 2 * (size_t)R * H;         // [H][H] (MLDS)
  const long p0 = (long)blockIdx.x * R;
  const int rows = (int)min((long)R, (long)tb.B - p0);
  const int items = rows * H;
  const int tid = threadIdx.x;
  const int* __restrict__ off = tb.off;
  const int Tw = tb.lens[tb.perm[p0]];   // the longest row of this workgroup
  if (MLDS)
    for (int e = tid; e < H * H; e += RAG_THREADS) Ml[e] = a.M[e];
  const S* M = MLDS ? Ml : a.M;
  // v_{-1}: the initial states (forward; Sp block 0 holds all B sorted sequences) or zero (reverse), in both buffers
  for (int e = tid; e < items; e += RAG_THREADS) {
    v[e] = REV ? S(0) : a.Sp[p0 * H + e];
    v[(size_t)R * H + e] = S(0);
  }
  int rq[RAG_QMAX], jq[RAG_QMAX], lq[RAG_QMAX];
  S pre[RAG_QMAX];
  const int t0 = REV ? Tw - 1 : 0;
#pragma unroll
  for (int q = 0; q < RAG_QMAX; ++q) {
    const int item = tid + q * RAG_THREADS;
    rq[q] = item / H;
    jq[q] = item - rq[q] * H;
    lq[q] = item < items ? tb.lens[tb.perm[p0 + rq[q]]] : 0;
    pre[q] = t0 < lq[q] ? a.Z[((long)off[t0] + p0 + rq[q]) * H + jq[q]] : S(0);
  }
  __syncthreads();
  int cur = 0;
  for (int step = 0; step < Tw; ++step) {
    const int t = REV ? Tw - 1 - step : step;
    const int tn = REV ? t - 1 : t + 1;  // the next step of the loop
    const long row_t = (long)off[t] + p0;
    const long row_n = tn >= 0 && tn < Tw ? (long)off[tn] + p0 : 0;
    const S* vc = v + (size_t)cur * R * H;
    S* vn = v + (size_t)(cur ^ 1) * R * H;
#pragma unroll
    for (int q = 0; q < RAG_QMAX; ++q) {
      const int item = tid + q * RAG_THREADS;
      if (t < lq[q]) {   // (lq is 0 beyond the workgroup's items)
        const int r = rq[q], j = jq[q];
        const long at_t = (row_t + r) * H + j;
        S acc = S(0);
        if (!REV || t + 1 < lq[q]) {
          const S* vr = vc + (size_t)r * H;
          const S* mj = M + j;
#pragma unroll 4
          for (int k = 0; k < H; ++k) acc = dm::fma(vr[k], mj[(size_t)k * H], acc);
        }
        S o;
        if (!REV) {
          const S z = pre[q] + acc;
          a.Z[at_t] = z;
          if constexpr (ACT == ACT_KIND_TANH) o = dm::tanh_act(z);
          else o = dm::logistic(z);
          a.Sa[at_t] = o;
        } else {
          const S h = a.Sa[at_t];
          if constexpr (ACT == ACT_KIND_TANH) o = dm::fma(acc, dm::tanh_dact(h), pre[q]);
          else o = dm::fma(acc * h, S(1) - h, pre[q]);
          a.Z[at_t] = o;
        }
        vn[item] = o;
        if (tn >= 0 && tn < lq[q]) {   // the row is active at the next step too
          const long at_n = (row_n + r) * H + j;
          if (!REV) a.Sp[at_n] = o;
          pre[q] = a.Z[at_n];          // the next step's addend, loaded under the barrier
        }
      } else if (REV && tn >= 0 && tn == lq[q] - 1) {
        pre[q] = a.Z[(row_n + rq[q]) * H + jq[q]];   // the row joins at the next step
      }
    }
    __syncthreads();
    cur ^= 1;
  }
}

template <class S, bool REV, bool MLDS, int ACT>
void go(const RnnSeqPlan& p, const RaggedTables& tb, const void* M, void* Z, void* Sa, void* Sp, int64_t H, hipStream_t s) {
  static bool attr = false;
  if (!attr) {
    TO_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(rnn_ragged_seq_kernel<S, REV, MLDS, ACT>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)RAG_LDS_MAX));
    attr = true;
  }
  RaggedSeqArgs<S> a{(const S*)M, (S*)Z, (S*)Sa, (S*)Sp, (int)H, p.R};
  launch_k(rnn_ragged_seq_kernel<S, REV, MLDS, ACT>, dim3((unsigned)p.grid), dim3(RAG_THREADS), p.lds, s, a, tb);
}

template <class S, bool REV, bool MLDS>
void go_act(int act_kind, const RnnSeqPlan& p, const RaggedTables& tb, const void* M, void* Z, void* Sa, void* Sp, int64_t H,
            hipStream_t s) {
  if (act_kind == ACT_KIND_TANH) go<S, REV, MLDS, ACT_KIND_TANH>(p, tb, M, Z, Sa, Sp, H, s);
  else go<S, REV, MLDS, ACT_KIND_LOGISTIC>(p, tb, M, Z, Sa, Sp, H, s);
}

unsigned blocks_for(int64_t total) {
  int64_t b = (total + RAG_THREADS - 1) / RAG_THREADS;
  return (unsigned)std::min<int64_t>(std::max<int64_t>(b, 1), 4096);   // the rest by grid stride
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace

void launch_ragged_pack(int dtype, const RaggedTables& tb, const void* src, int64_t sb, int64_t st, int64_t sj, void* dst,
                        int64_t n, hipStream_t s) {
  if (tb.N == 0 || n == 0) return;
  const int64_t es = dtype == TO_F64 ? 8 : 4;
  const char* sp = static_cast<const char*>(src);
  const bool wide = sj == 1 && (n * es) % 16 == 0 && (sb * es) % 16 == 0 && (st * es) % 16 == 0 && aligned16(src) && aligned16(dst);
  if (wide) {
    const int64_t npr = n * es / 16;
    launch_k(ragged_pack_kernel<Piece16>, dim3(blocks_for(tb.N * npr)), dim3(RAG_THREADS), 0, s, sp, static_cast<Piece16*>(dst),
             tb, (long)(sb * es), (long)(st * es), 1L, (long)npr);
  } else if (es == 8) {
    launch_k(ragged_pack_kernel<unsigned long long>, dim3(blocks_for(tb.N * n)), dim3(RAG_THREADS), 0, s, sp,
             static_cast<unsigned long long*>(dst), tb, (long)(sb * es), (long)(st * es), (long)sj, (long)n);
  } else {
    launch_k(ragged_pack_kernel<unsigned>, dim3(blocks_for(tb.N * n)), dim3(RAG_THREADS), 0, s, sp, static_cast<unsigned*>(dst),
             tb, (long)(sb * es), (long)(st * es), (long)sj, (long)n);
  }
  TO_HIP(hipGetLastError());
  count_launch();
}

void launch_ragged_unpack(int dtype, const RaggedTables& tb, const void* src, void* dst, int64_t T, int64_t n, hipStream_t s) {
  if (tb.B == 0 || T == 0 || n == 0) return;
  const int64_t es = dtype == TO_F64 ? 8 : 4;
  if ((n * es) % 16 == 0 && aligned16(src) && aligned16(dst)) {
    const int64_t npr = n * es / 16;
    launch_k(ragged_unpack_kernel<Piece16>, dim3(blocks_for(tb.B * T * npr)), dim3(RAG_THREADS), 0, s,
             static_cast<const Piece16*>(src), static_cast<Piece16*>(dst), tb, (long)T, (long)npr);
  } else if (es == 8) {
    launch_k(ragged_unpack_kernel<unsigned long long>, dim3(blocks_for(tb.B * T * n)), dim3(RAG_THREADS), 0, s,
             static_cast<const unsigned long long*>(src), static_cast<unsigned long long*>(dst), tb, (long)T, (long)n);
  } else {
    launch_k(ragged_unpack_kernel<unsigned>, dim3(blocks_for(tb.B * T * n)), dim3(RAG_THREADS), 0, s,
             static_cast<const unsigned*>(src), static_cast<unsigned*>(dst), tb, (long)T, (long)n);
  }
  TO_HIP(hipGetLastError());
  count_launch();
}

void launch_ragged_states(int dtype, int mode, const RaggedTables& tb, const void* src, void* dst, int64_t n, int64_t sb,
                          int64_t ss, hipStream_t s) {
  TO_CHECK(mode >= 0 && mode <= 2, TO_ERR_STATE, "internal: ragged state mover");
  const int64_t rows = mode == 2 ? (int64_t)tb.N - tb.B : (int64_t)tb.B;
  if (rows <= 0 || n == 0) return;
  const dim3 grid(blocks_for(rows * n)), block(RAG_THREADS);
#define TOPS_RAG_STATE(S, MODE)                                                                                          \
  launch_k(ragged_state_kernel<S, MODE>, grid, block, 0, s, static_cast<const S*>(src), static_cast<S*>(dst), tb, (long)n, \
           (long)sb, (long)ss)
#define TOPS_RAG_STATE_OF(S)                                                                                             \
  do {                                                                                                                   \
    if (mode == 0) TOPS_RAG_STATE(S, 0); else if (mode == 1) TOPS_RAG_STATE(S, 1); else TOPS_RAG_STATE(S, 2);            \
  } while (0)
  if (dtype == TO_F64) TOPS_RAG_STATE_OF(double);
  else TOPS_RAG_STATE_OF(float);
#undef TOPS_RAG_STATE_OF
#undef TOPS_RAG_STATE
  TO_HIP(hipGetLastError());
  count_launch();
}

void launch_rnn_ragged_seq(int dtype, bool reverse, const RnnSeqPlan& p, const RaggedTables& tb, const void* M, void* Z,
                           void* Sa, void* Sp, int64_t H, int act_kind, hipStream_t s) {
  if (tb.B == 0 || tb.N == 0) return;
  TO_CHECK(act_kind == ACT_KIND_LOGISTIC || act_kind == ACT_KIND_TANH, TO_ERR_ARG, "rnn_ragged: unknown state activation");
  const int k = act_kind;
  if (dtype == TO_F64) {
    if (reverse) p.m_lds ? go_act<double, true, true>(k, p, tb, M, Z, Sa, Sp, H, s) : go_act<double, true, false>(k, p, tb, M, Z, Sa, Sp, H, s);
    else p.m_lds ? go_act<double, false, true>(k, p, tb, M, Z, Sa, Sp, H, s) : go_act<double, false, false>(k, p, tb, M, Z, Sa, Sp, H, s);
  } else {
    if (reverse) p.m_lds ? go_act<float, true, true>(k, p, tb, M, Z, Sa, Sp, H, s) : go_act<float, true, false>(k, p, tb, M, Z, Sa, Sp, H, s);
    else p.m_lds ? go_act<float, false, true>(k, p, tb, M, Z, Sa, Sp, H, s) : go_act<float, false, false>(k, p, tb, M, Z, Sa, Sp, H, s);
  }
  TO_HIP(hipGetLastError());
  count_launch();
}

}  // namespace to
