// The reconstruction head of to_autoencoder_stack_*: everything behind the last layer's contraction, per row.  In an
// autoencoder the head is as wide as the input (784 in the reference's data) and it is the only per-row work of a step that
// is not a GEMM.  With v = z + bias (bias optional), a = act(v) and t the target row (in `trainEncoder` the input row itself,
// AutoEncoder.hs:130-137):
//   pair 1  softmax  >>> crossEntropy : a = exp(v - max v) / sum,  dz = a * sum(t) - t,  loss = -sum t log a
//   pair 2  logistic >>> squaredError : dz = 2 (a - t) a (1 - a),                        loss = sum (a - t)^2
//   pair 3  tanh     >>> squaredError : dz = 2 (a - t) (1 - a^2)
//   pair 4  identity >>> squaredError : dz = 2 (a - t)
// Three optional outputs: dz (may be z itself), out = a (may be z itself; dz and out are different buffers), loss [B].
// Without a target (decode) t counts as 0 and only `out` means anything.
//
// One wave per row, four rows per workgroup; nothing crosses a wave: no LDS, no barrier, no atomics.  A row of up to
// RECON_TILE = 1,024 elements is held in registers -- z and the target are read once, each output is written once; wider rows
// go tile by tile (softmax: three sweeps over z, the last one writing).  Lane i of a tile holds the 16-byte pieces
// i, i + 64, ...: one 16-byte load / store per piece where the row bytes and every base allow (VEC), the same elements one at
// a time otherwise -- so which lane adds which element, and with it every bit of the result, does not depend on alignment.
#include "common.hpp"
#include "devmath.hpp"

namespace to {
namespace {

constexpr int RECON_TILE = 1024;

template <class S>
struct alignas(16) Piece {
  S v[16 / sizeof(S)];
};

// Not dm::wave_max: compare-select keeps the value held where the other one is a NaN; fmax would drop the NaN.
template <class S>
__device__ __forceinline__ S rh_wmax(S v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const S o = __shfl_xor(v, off, 64);
    v = o > v ? o : v;
  }
  return v;
}

// a = act(v) of the three elementwise pairs, and act' written on a
template <int PAIR, class S>
__device__ __forceinline__ S rh_act(S v) {
  if constexpr (PAIR == 2) return dm::logistic(v);
  else if constexpr (PAIR == 3) return dm::tanh_act(v);
  else return v;
}
template <int PAIR, class S>
__device__ __forceinline__ S rh_dact(S a) {
  if constexpr (PAIR == 2) return a * (S(1) - a);
  else if constexpr (PAIR == 3) return dm::tanh_dact(a);
  else return S(1);
}

// One tile of a row in registers: slot (c, e) is element base + (c * 64 + lane) * V + e of the row.
template <class S, bool VEC>
struct Tile {
  static constexpr int V = 16 / sizeof(S), NC = RECON_TILE / (64 * V);
  S x[NC][V];

  __device__ __forceinline__ static int col(int base, int lane, int c) { return base + (c * 64 + lane) * V; }

  // x = p[...] (+ q[...] when q is given); slots beyond n hold `fill`.  p null: all `fill`.
  __device__ __forceinline__ void load(const S* p, const S* q, int base, int n, int lane, S fill) {
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const int j = col(base, lane, c);
#pragma unroll
      for (int e = 0; e < V; ++e) x[c][e] = fill;
      if (!p || j >= n) continue;
      if constexpr (VEC) {  // (n is a multiple of V: a piece is inside the row or outside it)
        const Piece<S> a = *reinterpret_cast<const Piece<S>*>(p + j);
#pragma unroll
        for (int e = 0; e < V; ++e) x[c][e] = a.v[e];
        if (q) {
          const Piece<S> b = *reinterpret_cast<const Piece<S>*>(q + j);
#pragma unroll
          for (int e = 0; e < V; ++e) x[c][e] += b.v[e];
        }
      } else {
#pragma unroll
        for (int e = 0; e < V; ++e)
          if (j + e < n) x[c][e] = q ? p[j + e] + q[j + e] : p[j + e];
      }
    }
  }
  __device__ __forceinline__ void store(S* p, int base, int n, int lane) const {
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const int j = col(base, lane, c);
      if (j >= n) continue;
      if constexpr (VEC) {
        Piece<S> a;
#pragma unroll
        for (int e = 0; e < V; ++e) a.v[e] = x[c][e];
        *reinterpret_cast<Piece<S>*>(p + j) = a;
      } else {
#pragma unroll
        for (int e = 0; e < V; ++e)
          if (j + e < n) p[j + e] = x[c][e];
      }
    }
  }
  __device__ __forceinline__ bool in(int base, int n, int lane, int c, int e) const { return col(base, lane, c) + e < n; }
};

// z [B, n] contiguous; target rows t_sm elements apart (null: none); dz, out [B, n] contiguous; loss [B]
template <class S, int PAIR, bool VEC>
__global__ __launch_bounds__(256) void recon_head_kernel(const S* z, const S* __restrict__ bias, const S* t, long t_sm, S* dz,
                                                         S* out, S* __restrict__ loss, long B, int n) {
  using T = Tile<S, VEC>;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= B) return;  // (a whole wave: no barrier follows)
  const int lane = threadIdx.x & 63;
  const S* zr = z + row * n;
  const S* tr = t ? t + row * t_sm : nullptr;
  S* dr = dz ? dz + row * n : nullptr;
  S* outr = out ? out + row * n : nullptr;
  const bool one = n <= RECON_TILE;  // the row is loaded once and stays in registers
  T v, y;
  S l = S(0);
  if constexpr (PAIR == 1) {
    // subtracting the row maximum is the same value in exact arithmetic and avoids the overflow (as loss_grad_rows_kernel)
    S mx = S(-INFINITY);
    for (int base = 0; base < n; base += RECON_TILE) {
      v.load(zr, bias, base, n, lane, S(-INFINITY));
#pragma unroll
      for (int c = 0; c < T::NC; ++c)
#pragma unroll
        for (int e = 0; e < T::V; ++e) mx = v.x[c][e] > mx ? v.x[c][e] : mx;
    }
    mx = rh_wmax(mx);
    S se = S(0), st = S(0);
    for (int base = 0; base < n; base += RECON_TILE) {
      if (!one) v.load(zr, bias, base, n, lane, S(-INFINITY));
      y.load(tr, nullptr, base, n, lane, S(0));
#pragma unroll
      for (int c = 0; c < T::NC; ++c)
#pragma unroll
        for (int e = 0; e < T::V; ++e) {
          if (v.in(base, n, lane, c, e)) se += dm::exp(v.x[c][e] - mx);
          st += y.x[c][e];
        }
    }
    se = dm::wave_sum(se);
    st = dm::wave_sum(st);
    const S inv = S(1) / se, lse = dm::log(se);
    for (int base = 0; base < n; base += RECON_TILE) {
      if (!one) {
        v.load(zr, bias, base, n, lane, S(-INFINITY));
        y.load(tr, nullptr, base, n, lane, S(0));
      }
#pragma unroll
      for (int c = 0; c < T::NC; ++c)
#pragma unroll
        for (int e = 0; e < T::V; ++e) {
          if (!v.in(base, n, lane, c, e)) continue;
          const S d = v.x[c][e] - mx, p = dm::exp(d) * inv, tt = y.x[c][e];
          l += dm::ce_term(tt, d, lse);  // (not -tt log p: finite where p underflows)
          v.x[c][e] = p;
          y.x[c][e] = p * st - tt;
        }
      if (outr) v.store(outr, base, n, lane);
      if (dr) y.store(dr, base, n, lane);
    }
  } else {
    for (int base = 0; base < n; base += RECON_TILE) {
      v.load(zr, bias, base, n, lane, S(0));
      y.load(tr, nullptr, base, n, lane, S(0));
#pragma unroll
      for (int c = 0; c < T::NC; ++c)
#pragma unroll
        for (int e = 0; e < T::V; ++e) {
          if (!v.in(base, n, lane, c, e)) continue;
          const S a = rh_act<PAIR>(v.x[c][e]), d = a - y.x[c][e];
          l += d * d;
          v.x[c][e] = a;
          y.x[c][e] = S(2) * d * rh_dact<PAIR>(a);
        }
      if (outr) v.store(outr, base, n, lane);
      if (dr) y.store(dr, base, n, lane);
    }
  }
  if (loss) {
    l = dm::wave_sum(l);
    if (lane == 0) loss[row] = l;
  }
}

template <class S, int PAIR>
void recon_launch(const void* z, const void* bias, const void* t, int64_t t_sm, void* dz, void* out, void* loss, int64_t B,
                  int64_t n, hipStream_t s) {
  auto al = [](const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; };
  const int64_t es = (int64_t)sizeof(S);
  const bool vec = (n * es) % 16 == 0 && al(z) && al(bias) && al(dz) && al(out) && al(t) && (!t || B == 1 || (t_sm * es) % 16 == 0);
  const dim3 grid((unsigned)((B + 3) / 4)), block(256);
  if (vec)
    launch_k(recon_head_kernel<S, PAIR, true>, grid, block, 0, s, (const S*)z, (const S*)bias, (const S*)t, (long)t_sm, (S*)dz,
             (S*)out, (S*)loss, (long)B, (int)n);
  else
    launch_k(recon_head_kernel<S, PAIR, false>, grid, block, 0, s, (const S*)z, (const S*)bias, (const S*)t, (long)t_sm, (S*)dz,
             (S*)out, (S*)loss, (long)B, (int)n);
}

}  // namespace

void launch_recon_head(int dtype, int pair, const void* z, const void* bias, const void* target, int64_t t_sm, void* dz,
                       void* out, void* loss, int64_t B, int64_t n, hipStream_t s) {
  TO_CHECK(pair >= 1 && pair <= 4, TO_ERR_STATE, "internal: reconstruction head: unknown pair");
  TO_CHECK(n <= 2147483647LL - RECON_TILE && B <= 4LL * 2147483647LL, TO_ERR_SHAPE, "reconstruction head: too wide or too many rows");
  TO_CHECK(!(dz && dz == out), TO_ERR_STATE, "internal: reconstruction head: dz and out are one buffer");
  if (B == 0 || n == 0) return;
  auto go = [&](auto* tag) {
    using S = std::remove_pointer_t<decltype(tag)>;
    switch (pair) {
      case 1: recon_launch<S, 1>(z, bias, target, t_sm, dz, out, loss, B, n, s); break;
      case 2: recon_launch<S, 2>(z, bias, target, t_sm, dz, out, loss, B, n, s); break;
      case 3: recon_launch<S, 3>(z, bias, target, t_sm, dz, out, loss, B, n, s); break;
      default: recon_launch<S, 4>(z, bias, target, t_sm, dz, out, loss, B, n, s); break;
    }
  };
  if (dtype == TO_F64) go((double*)nullptr);
  else go((float*)nullptr);
  TO_HIP(hipGetLastError());
  count_launch();
}

}  // namespace to
