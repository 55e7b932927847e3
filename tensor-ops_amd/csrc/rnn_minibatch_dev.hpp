// What the two minibatch BPTT kernels share (rnn_minibatch.hip: every sequence T steps long, row r = t * Mp + q;
// rnn_minibatch_ragged.hip: sequences of their own lengths, the rows of a step packed): the workgroup's shape, the 16 x 16 x 4
// MFMA block and its fragment layout, the kernel's arguments -- the LDS map and the tape record of rnn_minibatch_plan
// (common.hpp) with the stack's pointers --, how the host fills them, and the update's row reduction.
#pragma once
#include <type_traits>

#include "common.hpp"
#include "devmath.hpp"

namespace to {

namespace {

constexpr int MB_THREADS = 512, MB_NW = MB_THREADS / 64;

typedef float mb_f32x4 __attribute__((ext_vector_type(4)));
typedef double mb_f64x4 __attribute__((ext_vector_type(4)));
template <class S> using mb_v4 = typename std::conditional<sizeof(S) == 8, mb_f64x4, mb_f32x4>::type;
// A lane l = A[i = l & 15][k = l >> 4], B lane l = B[k = l >> 4][j = l & 15]
__device__ __forceinline__ mb_f32x4 mb_mfma(float a, float b, mb_f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
__device__ __forceinline__ mb_f64x4 mb_mfma(double a, double b, mb_f64x4 c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }
// D register r of lane l (g = l >> 4) is row 4 g + r (fp32) or g + 4 r (fp64), column l & 15
template <class S> __device__ __forceinline__ int mb_row(int g, int r) { return sizeof(S) == 8 ? g + 4 * r : 4 * g + r; }

template <class S>
struct RnnMinibatchArgs {
  S* W[RNN_GEN_MAX_LAYERS];    // [n_l][n_{l-1}]
  S* WS[RNN_GEN_MAX_LAYERS];   // [n_l][n_l] (stateful)
  S* b[RNN_GEN_MAX_LAYERS];
  S* s[RNN_GEN_MAX_LAYERS];    // [n_l] (stateful): the learned initial state
  int n[RNN_GEN_MAX_LAYERS + 1];
  int sk[RNN_GEN_MAX_LAYERS];  // state activation, -1: stateless
  // LDS offsets (elements): W k-major [up4(m)][ld], W' k-major [up4(n)][ld], b and s [up4(n)]
  int w_off[RNN_GEN_MAX_LAYERS], ws_off[RNN_GEN_MAX_LAYERS], b_off[RNN_GEN_MAX_LAYERS], s_off[RNN_GEN_MAX_LAYERS],
      ld[RNN_GEN_MAX_LAYERS];
  // offsets within one row's tape record: the layer's input row, its state S_t, its z_t / dz_t
  int t_in[RNN_GEN_MAX_LAYERS], t_s[RNN_GEN_MAX_LAYERS], t_dz[RNN_GEN_MAX_LAYERS];
  const S* X;             // [N][T][n_0]
  const S* Y;             // [N][T][n_L]
  S* losses;              // [n_idx][T] or null
  const long long* idx;   // [n_idx] or null: sequences 0 .. n_idx-1
  S* tape;                // [T * Mp][rec]
  long n_idx, M, T, rec;
  int L, Mp, chain_off, hs, hidden_kind, softmax;
  S rate_state, rate_params;
};

// the plan and the operands of a call as the kernels read them
template <class S>
RnnMinibatchArgs<S> mb_args(const RnnMinibatchPlan& p, const RnnMinibatchOperands& o) {
  RnnMinibatchArgs<S> a{};
  for (int l = 0; l < o.L; ++l) {
    a.W[l] = (S*)o.W[l]; a.WS[l] = (S*)o.WS[l]; a.b[l] = (S*)o.b[l]; a.s[l] = (S*)o.s[l];
    a.sk[l] = o.state_kind[l];
    a.w_off[l] = p.w_off[l]; a.ws_off[l] = p.ws_off[l]; a.b_off[l] = p.b_off[l]; a.s_off[l] = p.s_off[l]; a.ld[l] = p.ld[l];
    a.t_in[l] = p.t_in[l]; a.t_s[l] = p.t_s[l]; a.t_dz[l] = p.t_dz[l];
  }
  for (int l = 0; l <= o.L; ++l) a.n[l] = (int)o.widths[l];
  a.X = (const S*)o.X; a.Y = (const S*)o.Y; a.losses = (S*)o.losses; a.idx = o.idx; a.tape = (S*)o.tape;
  a.n_idx = (long)o.n_idx; a.M = (long)o.M; a.T = (long)o.T; a.rec = (long)p.rec;
  a.L = o.L; a.Mp = p.Mp; a.chain_off = p.chain_off; a.hs = p.hs; a.hidden_kind = o.hidden_kind;
  a.softmax = o.softmax ? 1 : 0;
  a.rate_state = (S)o.rate_state; a.rate_params = (S)o.rate_params;
  return a;
}

// One k-major matrix's update: M[k][j] -= rate * sum over ascending r of src[r][k] dz[r][j], k < m, j < n.  The 16 x 16
// output blocks are dealt to the waves; the reduction runs over the rows, four an MFMA (lane group g takes row r + g).
template <class S>
__device__ __forceinline__ void mb_update(const S* tape, long rec, long R, int osrc, int odz, int m, int n, int ld, S* Mk, S rate,
                                          int wave, int c, int g) {
  const int m4 = (m + 3) & ~3, n4 = (n + 3) & ~3, ncb = (n + 15) >> 4, nkb = (m + 15) >> 4;
  for (int it = wave; it < nkb * ncb; it += MB_NW) {
    const int kb = it / ncb, cb = it - kb * ncb, ka = kb * 16 + c, jb = cb * 16 + c;
    const bool ina = ka < m4, inb = jb < n4;
    mb_v4<S> acc = {S(0), S(0), S(0), S(0)};
    const S* p = tape + g * rec;
    for (long r = 0; r < R; r += 16, p += 16 * rec) {   // R is a multiple of 16: four MFMAs' loads in flight together
      S av[4], bv[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        av[u] = ina ? p[u * 4 * rec + osrc + ka] : S(0);
        bv[u] = inb ? p[u * 4 * rec + odz + jb] : S(0);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) acc = mb_mfma(av[u], bv[u], acc);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int k = kb * 16 + mb_row<S>(g, r);
      if (k < m && jb < n) Mk[k * ld + jb] -= rate * acc[r];
    }
  }
}

// The stack between global memory and LDS, once a launch each way: zeros everywhere below the chain blocks, then every
// layer's W and W' k-major, b and the learned initial states (rnn_minibatch_ragged.hip; rnn_minibatch.hip spells the same
// loops out in its kernel)
template <class S>
__device__ __forceinline__ void mb_stack_in(const RnnMinibatchArgs<S>& a, S* lds, int tid) {
  for (int e = tid; e < a.chain_off; e += MB_THREADS) lds[e] = S(0);
  __syncthreads();
  for (int l = 0; l < a.L; ++l) {
    const int m = a.n[l], n = a.n[l + 1], ld = a.ld[l];
    for (int e = tid; e < n * m; e += MB_THREADS) lds[a.w_off[l] + (e % m) * ld + e / m] = a.W[l][e];
    if (a.sk[l] >= 0) {
      for (int e = tid; e < n * n; e += MB_THREADS) lds[a.ws_off[l] + (e % n) * ld + e / n] = a.WS[l][e];
      for (int e = tid; e < n; e += MB_THREADS) lds[a.s_off[l] + e] = a.s[l][e];
    }
    for (int e = tid; e < n; e += MB_THREADS) lds[a.b_off[l] + e] = a.b[l][e];
  }
  __syncthreads();
}
template <class S>
__device__ __forceinline__ void mb_stack_out(const RnnMinibatchArgs<S>& a, const S* lds, int tid) {
  for (int l = 0; l < a.L; ++l) {
    const int m = a.n[l], n = a.n[l + 1], ld = a.ld[l];
    for (int e = tid; e < n * m; e += MB_THREADS) a.W[l][e] = lds[a.w_off[l] + (e % m) * ld + e / m];
    if (a.sk[l] >= 0) {
      for (int e = tid; e < n * n; e += MB_THREADS) a.WS[l][e] = lds[a.ws_off[l] + (e % n) * ld + e / n];
      for (int e = tid; e < n; e += MB_THREADS) a.s[l][e] = lds[a.s_off[l] + e];
    }
    for (int e = tid; e < n; e += MB_THREADS) a.b[l][e] = lds[a.b_off[l] + e];
  }
}

}  // namespace

}  // namespace to
