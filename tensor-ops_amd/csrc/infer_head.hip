// The output head of batched inference (to_fflayer_stack_infer): `runNetwork`'s last layer (FeedForward.hs:123-129) and
// the validation folds of app/MNIST.hs:366-389 -- `TT.argMax` of every output row, the confusion matrix of
// (predicted, actual) -- per row, on the device.
//   infer_narrow_kernel : n_L <= 32 at any K.  out = act(A W^T + b) and the folds in ONE launch: A is streamed from HBM
//                         once (16-byte loads where the rows allow it), W_L sits in LDS (in K chunks when it does not
//                         fit), eight lanes share a row and the finished row stays within the wave for the epilogue.
//   infer_rows_kernel   : any n_L.  z (the last GEMM's output, bias not added) -> bias, softmax / logistic, store,
//                         argMax, confusion: one wave per row, looping over the row in 64-wide chunks.
//   bias_act_kernel     : a hidden layer whose GEMM has no fused epilogue (the tiled fp64 kernel): h = act(z + b), act
//                         logistic or tanh (a template parameter), in place, one elementwise launch (what the planner
//                         does then, lazy.cpp).
// argMax follows arg_max_rows_kernel (reduce_layout.hip) exactly -- the same per-lane fold and the same xor tree, and with a NaN
// in the row the same fold again over the elements behind the last NaN -- so a class id is bit for bit what to_arg_max returns
// for the stored row, ties (earliest index) and NaN included.
// Every reduction has a fixed order per row: a row's result does not depend on B or on where the row sits in the batch.
#include <algorithm>
#include <type_traits>

#include "common.hpp"
#include "devmath.hpp"

namespace to {

namespace {

#define TO_DISPATCH(dtype, CALL)                       \
  do {                                                 \
    if ((dtype) == TO_F64) { using S = double; CALL; } \
    else { using S = float; CALL; }                    \
  } while (0)

template <class S>
struct alignas(16) Vec16 {  // one 16-byte load: 4 floats / 2 doubles
  S v[16 / sizeof(S)];
};

// one step of arg_max_rows_kernel's tree: (best, bi) absorbs the partial winner (ob, oi); the left (smaller index) one
// wins unless the other is strictly greater, bi < 0 = empty
template <class S>
__device__ __forceinline__ void am_combine(S& best, int& bi, S ob, int oi) {
  if (oi >= 0 && (bi < 0 || (oi < bi ? !(ob < best) : !(best >= ob)))) { best = ob; bi = oi; }
}

// what lane 0 of arg_max_rows_kernel ends with for a row of n <= NP <= 32 values (value j on lane j, one each): the
// tree's steps with offsets >= NP only meet empty lanes, the later ones are replayed here for the lanes that reach lane 0.
// As there, the elements up to the last NaN of the row are out of the fold, and n - 1 is the answer when nothing is left.
template <class S, int NP>
__device__ __forceinline__ int arg_max_tree(const S (&v)[NP], int n) {
  S b[NP];
  int bi[NP];
  int ln = -1;
#pragma unroll
  for (int j = 0; j < NP; ++j)
    if (j < n && v[j] != v[j]) ln = j;
#pragma unroll
  for (int j = 0; j < NP; ++j) { b[j] = v[j]; bi[j] = (j < n && j > ln) ? j : -1; }
#pragma unroll
  for (int off = NP / 2; off > 0; off >>= 1)
#pragma unroll
    for (int j = 0; j < off; ++j) am_combine(b[j], bi[j], b[j + off], bi[j + off]);
  return bi[0] < 0 ? n - 1 : bi[0];
}

constexpr int NARROW_LANES = 8;                 // lanes per row
constexpr int NARROW_ROWS = 256 / NARROW_LANES; // rows per workgroup pass
constexpr int NARROW_UNROLL = 4;                // 16-byte loads in flight per lane

// Lane `sub` of a row's eight owns the 16-byte pieces k / V = sub (mod 8) of the row and accumulates them in increasing
// k; the eight partial sums meet in an xor tree.  The assignment depends on k alone (chunks start at multiples of 8 V),
// and the scalar path (ragged rows, offset views) loads the same elements in the same order: same bits either way.
template <class S, int NP>
__global__ __launch_bounds__(256) void infer_narrow_kernel(const S* __restrict__ A, long a_sm, long B, long K,
                                                           const S* __restrict__ W, const S* __restrict__ bias, int n,
                                                           int softmax, long Kc, int vec, S* __restrict__ out,
                                                           const S* __restrict__ y, long y_sm, int* __restrict__ classes,
                                                           unsigned long long* __restrict__ conf) {
  constexpr int V = 16 / sizeof(S);
  constexpr int STEP = NARROW_LANES * V;   // elements of a row per pass of its eight lanes
  extern __shared__ __align__(16) unsigned char lds_raw[];
  S* Wl = reinterpret_cast<S*>(lds_raw);   // [n][Kc]: W_L[:, c0 .. c0 + Kc), zero beyond K
  __shared__ unsigned hist[NP * NP];
  const int tid = threadIdx.x, sub = tid & (NARROW_LANES - 1), grp = tid / NARROW_LANES;
  const bool one_chunk = Kc >= K;
  auto stage = [&](long c0) {
    const long kw = K - c0 < Kc ? K - c0 : Kc;
    for (long i = tid; i < (long)n * Kc; i += 256) {
      const long j = i / Kc, kk = i - j * Kc;
      Wl[i] = kk < kw ? W[j * K + c0 + kk] : S(0);
    }
  };
  if (conf)
    for (int i = tid; i < n * n; i += 256) hist[i] = 0;
  if (one_chunk) stage(0);
  __syncthreads();
  for (long r0 = (long)blockIdx.x * NARROW_ROWS; r0 < B; r0 += (long)gridDim.x * NARROW_ROWS) {
    const long row = r0 + grp;
    const bool live = row < B;
    S acc[NP];
#pragma unroll
    for (int j = 0; j < NP; ++j) acc[j] = S(0);
    for (long c0 = 0; c0 < K; c0 += Kc) {
      if (!one_chunk) {
        __syncthreads();
        stage(c0);
        __syncthreads();
      }
      if (!live) continue;
      const long kw = K - c0 < Kc ? K - c0 : Kc;
      const S* a = A + row * a_sm + c0;
      for (long k = (long)sub * V; k < kw; k += (long)STEP * NARROW_UNROLL) {
        S av[NARROW_UNROLL][V];
#pragma unroll
        for (int u = 0; u < NARROW_UNROLL; ++u) {
          const long kk = k + (long)u * STEP;
          if (vec && kk + V <= kw) {
            const Vec16<S> t = *reinterpret_cast<const Vec16<S>*>(a + kk);
#pragma unroll
            for (int e = 0; e < V; ++e) av[u][e] = t.v[e];
          } else {
#pragma unroll
            for (int e = 0; e < V; ++e) av[u][e] = kk + e < kw ? a[kk + e] : S(0);
          }
        }
#pragma unroll
        for (int u = 0; u < NARROW_UNROLL; ++u) {
          const long kk = k + (long)u * STEP;
          if (kk >= kw) break;
#pragma unroll
          for (int j = 0; j < NP; ++j) {
            if (j >= n) break;
            const Vec16<S> w = *reinterpret_cast<const Vec16<S>*>(Wl + (long)j * Kc + kk);
#pragma unroll
            for (int e = 0; e < V; ++e) acc[j] = dm::fma(av[u][e], w.v[e], acc[j]);
          }
        }
      }
    }
    if (!live) continue;
    // the eight partial sums: every lane of the row ends with the same (commutative) sums
#pragma unroll
    for (int off = NARROW_LANES / 2; off > 0; off >>= 1)
#pragma unroll
      for (int j = 0; j < NP; ++j) acc[j] += __shfl_xor(acc[j], off, 64);
    S v[NP];
#pragma unroll
    for (int j = 0; j < NP; ++j) v[j] = j < n ? acc[j] + bias[j] : S(0);
    if (softmax) {  // the row maximum subtracted first, as the loss head does (gemm_small.hip)
      S mx = S(-INFINITY);
#pragma unroll
      for (int j = 0; j < NP; ++j)
        if (j < n) mx = dm::max(mx, v[j]);
      S se = S(0);
#pragma unroll
      for (int j = 0; j < NP; ++j)
        if (j < n) { v[j] = dm::exp(v[j] - mx); se += v[j]; }
#pragma unroll
      for (int j = 0; j < NP; ++j) v[j] = v[j] / se;
    } else {
#pragma unroll
      for (int j = 0; j < NP; ++j) v[j] = dm::logistic(v[j]);
    }
    if (out) {
      S* o = out + row * n;
#pragma unroll
      for (int j = 0; j < NP; ++j)
        if (j < n && (j & (NARROW_LANES - 1)) == sub) o[j] = v[j];
    }
    if (sub != 0) continue;
    const int pred = arg_max_tree<S, NP>(v, n);
    if (classes) classes[row] = pred;
    if (conf) {
      S t[NP];
#pragma unroll
      for (int j = 0; j < NP; ++j) t[j] = j < n ? y[row * y_sm + j] : S(0);
      atomicAdd(&hist[pred * n + arg_max_tree<S, NP>(t, n)], 1u);
    }
  }
  if (conf) {  // integer adds: the sum does not depend on the order the workgroups arrive in
    __syncthreads();
    for (int i = tid; i < n * n; i += 256)
      if (hist[i]) atomicAdd(&conf[i], (unsigned long long)hist[i]);
  }
}

// arg_max_rows_kernel's per-lane fold and xor tree over one wave (lane j holds elements j, j + 64, ...).  (best, bi) and ln
// -- the last NaN the lane met, -1: none -- come from the caller's pass over the row; with a NaN in the row the fold is taken
// again over the elements behind the last one, which val(j) gives once more.
template <class S, class F>
__device__ __forceinline__ int wave_arg_max(S best, long bi, long ln, int n, int lane, F val) {
  if (__ballot(ln >= 0)) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const long ol = __shfl_xor((long long)ln, off, 64);
      ln = ol > ln ? ol : ln;
    }
    best = S(0);
    bi = -1;
    for (int j = lane; j < n; j += 64) {
      if (j <= ln) continue;
      const S v = val(j);
      if (bi < 0 || !(best >= v)) { best = v; bi = j; }
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const S ob = __shfl_xor(best, off, 64);
    const long oi = __shfl_xor((long long)bi, off, 64);
    if (oi >= 0 && (bi < 0 || (oi < bi ? !(ob < best) : !(best >= ob)))) { best = ob; bi = oi; }
  }
  return bi < 0 ? n - 1 : (int)bi;
}

// z and out may be the same buffer (each element is read, then written, by the same lane)
template <class S>
__global__ __launch_bounds__(256) void infer_rows_kernel(const S* z, long B, const S* __restrict__ bias, int n,
                                                         int softmax, S* out, const S* __restrict__ y, long y_sm,
                                                         int* __restrict__ classes, unsigned long long* __restrict__ conf) {
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= B) return;
  const int lane = threadIdx.x & 63;
  const S* zr = z + row * n;
  S mx = S(-INFINITY), se = S(0);
  if (softmax) {
    for (int j = lane; j < n; j += 64) mx = dm::max(mx, zr[j] + bias[j]);
    mx = dm::wave_max(mx);
    for (int j = lane; j < n; j += 64) se += dm::exp(zr[j] + bias[j] - mx);
    se = dm::wave_sum(se);
  }
  S best = S(0);
  long bi = -1, ln = -1;
  auto prob = [&](int j) {
    const S v = zr[j] + bias[j];
    return softmax ? dm::exp(v - mx) / se : dm::logistic(v);
  };
  for (int j = lane; j < n; j += 64) {
    const S p = prob(j);
    if (out) out[row * n + j] = p;
    if (p != p) ln = j;
    if (bi < 0 || !(best >= p)) { best = p; bi = j; }
  }
  // (out may be z: what this lane stored there is then the value, z itself where nothing was stored)
  const int pred = wave_arg_max(best, bi, ln, n, lane, [&](int j) { return out ? out[row * n + j] : prob(j); });
  int actual = 0;
  if (conf) {
    const S* yr = y + row * y_sm;
    best = S(0);
    bi = -1;
    ln = -1;
    for (int j = lane; j < n; j += 64) {
      const S t = yr[j];
      if (t != t) ln = j;
      if (bi < 0 || !(best >= t)) { best = t; bi = j; }
    }
    actual = wave_arg_max(best, bi, ln, n, lane, [&](int j) { return yr[j]; });
  }
  if (lane != 0) return;
  if (classes) classes[row] = pred;
  if (conf) atomicAdd(&conf[(long)pred * n + actual], 1ull);
}

template <class S, int ACT>
__global__ __launch_bounds__(256) void bias_act_kernel(S* __restrict__ x, const S* __restrict__ bias, long total, long n) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    if constexpr (ACT == ACT_KIND_TANH) x[i] = dm::tanh_act(x[i] + bias[i % n]);
    else if constexpr (ACT == ACT_KIND_IDENTITY) x[i] = x[i] + bias[i % n];
    else x[i] = dm::logistic(x[i] + bias[i % n]);
  }
}

template <class S, int NP>
void narrow_launch(const void* A, int64_t a_sm, int64_t B, int64_t K, const void* W, const void* bias, int n,
                   bool softmax, void* out, const void* y, int64_t y_sm, int* classes, unsigned long long* conf,
                   hipStream_t s) {
  constexpr int64_t V = 16 / sizeof(S), STEP = NARROW_LANES * V;
  // W_L in chunks of at most 64 KiB (two workgroups a CU); a chunk is a multiple of a row pass so that the chunking
  // does not change which lane adds which element
  const int64_t budget = (65536 / ((int64_t)n * (int64_t)sizeof(S))) / STEP * STEP;
  const int64_t kfull = (K + STEP - 1) / STEP * STEP;
  const int64_t Kc = kfull < budget ? kfull : budget;
  const size_t lds = (size_t)n * Kc * sizeof(S);
  const bool vec = reinterpret_cast<uintptr_t>(A) % 16 == 0 && (B == 1 || (a_sm * (int64_t)sizeof(S)) % 16 == 0);
  const int64_t per_cu = std::min<int64_t>(8, (160 * 1024) / (int64_t)(lds + NP * NP * 4));
  const int64_t blocks = (B + NARROW_ROWS - 1) / NARROW_ROWS;
  const unsigned grid = (unsigned)std::min<int64_t>(blocks, 256 * std::max<int64_t>(per_cu, 1));
  launch_k(infer_narrow_kernel<S, NP>, dim3(grid), dim3(256), lds, s, (const S*)A, (long)a_sm, (long)B, (long)K,
           (const S*)W, (const S*)bias, n, softmax ? 1 : 0, (long)Kc, vec ? 1 : 0, (S*)out, (const S*)y, (long)y_sm,
           classes, conf);
}

}  // namespace

void launch_infer_narrow(int dtype, const void* A, int64_t a_sm, int64_t B, int64_t K, const void* W, const void* bias,
                         int n, bool softmax, void* out, const void* y, int64_t y_sm, int* classes,
                         unsigned long long* conf, hipStream_t s) {
  TO_CHECK(n >= 1 && n <= INFER_NARROW_MAX && K >= 1, TO_ERR_STATE, "internal: narrow head outside its range");
  if (B == 0) return;
  auto go = [&](auto* tag) {
    using S = std::remove_pointer_t<decltype(tag)>;
    if (n <= 8) narrow_launch<S, 8>(A, a_sm, B, K, W, bias, n, softmax, out, y, y_sm, classes, conf, s);
    else if (n <= 16) narrow_launch<S, 16>(A, a_sm, B, K, W, bias, n, softmax, out, y, y_sm, classes, conf, s);
    else narrow_launch<S, 32>(A, a_sm, B, K, W, bias, n, softmax, out, y, y_sm, classes, conf, s);
  };
  if (dtype == TO_F64) go((double*)nullptr);
  else go((float*)nullptr);
  TO_HIP(hipGetLastError());
  count_launch();
}

void launch_infer_rows(int dtype, const void* z, int64_t B, const void* bias, int n, bool softmax, void* out,
                       const void* y, int64_t y_sm, int* classes, unsigned long long* conf, hipStream_t s) {
  if (B == 0) return;
  TO_DISPATCH(dtype, launch_k(infer_rows_kernel<S>, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, s, (const S*)z, (long)B,
                              (const S*)bias, n, softmax ? 1 : 0, (S*)out, (const S*)y, (long)y_sm, classes, conf));
  TO_HIP(hipGetLastError());
  count_launch();
}

void launch_bias_act_rows(int dtype, void* x, const void* bias, int64_t B, int64_t n, int act_kind, hipStream_t s) {
  const int64_t total = B * n;
  if (total == 0) return;
  TO_CHECK(act_kind == ACT_KIND_LOGISTIC || act_kind == ACT_KIND_TANH || act_kind == ACT_KIND_IDENTITY, TO_ERR_ARG,
           "bias_act_rows: unknown activation");
  const unsigned grid = (unsigned)std::min<int64_t>((total + 255) / 256, 256 * 16);
  if (act_kind == ACT_KIND_TANH)
    TO_DISPATCH(dtype, launch_k(bias_act_kernel<S, ACT_KIND_TANH>, dim3(grid), dim3(256), 0, s, (S*)x, (const S*)bias,
                                (long)total, (long)n));
  else if (act_kind == ACT_KIND_IDENTITY)
    TO_DISPATCH(dtype, launch_k(bias_act_kernel<S, ACT_KIND_IDENTITY>, dim3(grid), dim3(256), 0, s, (S*)x, (const S*)bias,
                                (long)total, (long)n));
  else
    TO_DISPATCH(dtype, launch_k(bias_act_kernel<S, ACT_KIND_LOGISTIC>, dim3(grid), dim3(256), 0, s, (S*)x, (const S*)bias,
                                (long)total, (long)n));
  TO_HIP(hipGetLastError());
  count_launch();
}

}  // namespace to
