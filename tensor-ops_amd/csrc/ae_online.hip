// Per-sample `trainEncoder` (AutoEncoder.hs:87-110) folded over the rows of a data set as ONE persistent launch on ONE XCD:
// route B of to_autoencoder_stack_online_sgd.
//
// online_sgd.hip cannot hold an autoencoder: its head is at most 64 wide and it replicates every layer from the third on,
// while an autoencoder's output is as wide as its input and its last layer as large as its first.  The partition here is
// an hourglass, widest at both ends, over G <= 32 workgroups that keep what they own in LDS between samples (layers
// numbered from 1, widths i0 -> o1 -> .. -> oL = i0):
//
//   * layer 1 is split by ROWS: workgroup g owns W1[R_g, :], b1[R_g] and computes its slice of a1, one wave a row, the
//     sample's row prefetched into registers one sample ahead (i0 <= 2048);
//   * layer 2 is split by COLUMNS along the same R_g: workgroup g contributes W2[:, R_g] a1[R_g] -- o2 numbers -- to
//     EXCHANGE 1; every workgroup then sums the G partials in workgroup order (the same bits everywhere) and has z2;
//   * layers 3 .. L-1 are replicated: every workgroup computes and updates its own identical copy;
//   * layer L (L >= 3) is split by ROWS S_g of its outputs: a workgroup computes its slice of z_L, the head on it and its
//     part of the squared error, then contributes W_L[S_g, :]^T dz_L[S_g] -- o_{L-1} numbers -- and one more word, its loss
//     partial, to EXCHANGE 2; every workgroup sums those in workgroup order and walks the cotangent back through the
//     replicated layers to its own slice of dz1;
//   * L = 2: layer 2 IS the last layer; after exchange 1 every workgroup has all of z2 and runs the whole head
//     redundantly, there is no second exchange.
//
// Then `p - rate * g` in LDS on everything a workgroup holds; every cotangent was taken with the old weights.  Workgroup 0
// writes losses[j].  The three squaredError heads only: a row-split softmax would need a third exchange for the row's
// maximum and sum.
//
// The two exchanges, their watchdog and the commit are xcd_exchange.hpp's; a reader sums the words as they arrive, in
// registers: no landing area in LDS.  G = 1 touches none of this: no placement, no exchange through memory, no vote.
// Activations are a small per-layer switch (hidden, code and head activation of a layer may all differ); no hand-written
// instruction sequences: the wave sum is the shared butterfly.
#include "common.hpp"
#include "devmath.hpp"
#include "xcd_exchange.hpp"

namespace to {

namespace {

constexpr int AO_THREADS = 512, AO_NW = AO_THREADS / 64;
constexpr int AO_XREGS = 4;       // input elements prefetched per thread: i0 <= 2048
// red[0 .. 7]: a wave's part of a loss; [8]: a wait timed out (only ever set); [9]: the decision; [10]: G = 1's own loss partial
constexpr int AO_RED = 16, AO_FLAG = 8, AO_VERDICT = 9, AO_LOSS = 10;
constexpr int64_t AO_LDS_MAX = 160 * 1024;

template <class S>
struct AeOnlineArgs {
  int L;
  int dims[AE_ONLINE_MAX_LAYERS + 1];  // i0, o1 .. oL
  int kind[AE_ONLINE_MAX_LAYERS];      // ACT_KIND_* behind layer l + 1; kind[L - 1]: the head's activation
  S* W[AE_ONLINE_MAX_LAYERS];
  S* b[AE_ONLINE_MAX_LAYERS];
  const S* X;
  const long long* idx;  // sample order (device), or null: 0 .. n-1
  long n;
  S rate;
  S* losses;             // [n], or null
  int G, rpw, spw;       // workgroups; rows of layer 1 and (L >= 3) of layer L per workgroup
  unsigned long long* ex1;    // [2][G][o2][words of S]: {tag, 32 bits of the value}, zero at launch
  unsigned long long* ex2;    // [2][G][o_{L-1} + 1][words of S]
  unsigned long long* votes;  // 32 votes and the decision word, zero at launch
  int* status;           // host-visible: nonzero = a wait timed out at that sample + 1
  long long timeout;     // wall_clock64 ticks
};

template <class S> __device__ __forceinline__ S ao_act(int kind, S z) { return kind == ACT_KIND_IDENTITY ? z : dm::act(kind, z); }
template <class S> __device__ __forceinline__ S ao_dact(int kind, S h) { return kind == ACT_KIND_IDENTITY ? S(1) : dm::dact(kind, h); }

// Number j of every workgroup's contribution (ex: [G][n][WORDS]), summed in workgroup order -- every reader gets the same
// bits.  Four workgroups' words are in flight together; a word is asked for again until its tag says "this sample".
// (the poll is written out: on a shared primitive, in each shape tried, this file's assembly moves -- xcd_exchange.hpp)
template <class S>
__device__ __forceinline__ S ao_gather(const unsigned long long* ex, int G, int n, int j, unsigned tag, long long timeout, bool& ok) {
  constexpr int WORDS = sizeof(S) / 4;
  S sum = S(0.);
  if (!ok) return sum;   // (an earlier wait of this thread ran out: the sample is lost, no second watchdog period)
  const long long c0 = wall_clock64();
  for (int q0 = 0; q0 < G; q0 += 4) {
    unsigned long long v[4][WORDS];
    bool have[4][WORDS];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int w = 0; w < WORDS; ++w) { v[u][w] = 0ull; have[u][w] = q0 + u >= G; }
    while (true) {
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int w = 0; w < WORDS; ++w)
          if (!have[u][w])
            v[u][w] = __hip_atomic_load(ex + ((long)(q0 + u) * n + j) * WORDS + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      bool all = true;
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int w = 0; w < WORDS; ++w) {
          if (!have[u][w]) have[u][w] = (unsigned)(v[u][w] >> 32) == tag;
          all = all && have[u][w];
        }
      if (all) break;
      if (wall_clock64() - c0 > timeout) {
        ok = false;
        break;
      }
      __builtin_amdgcn_s_sleep(1);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (q0 + u < G) {
        unsigned wd[WORDS];
#pragma unroll
        for (int w = 0; w < WORDS; ++w) wd[w] = (unsigned)v[u][w];
        S x;
        __builtin_memcpy(&x, wd, sizeof(S));
        sum += x;
      }
  }
  return sum;
}

// (S = float or double)
template <class S>
__global__ __launch_bounds__(AO_THREADS) void ae_online_kernel(AeOnlineArgs<S> a) {
  const int G = a.G;
  if (G > 1 && (blockIdx.x & 7)) return;  // XCD 0 only; G = 1 is a grid of one workgroup, wherever it lands
  const int g = G > 1 ? (int)(blockIdx.x >> 3) : 0, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  const int L = a.L, i0 = a.dims[0], o1 = a.dims[1], o2 = a.dims[2], KL = a.dims[L - 1];
  const bool deep = L >= 3;
  const int r0 = g * a.rpw, nr = min(a.rpw, o1 - r0) > 0 ? min(a.rpw, o1 - r0) : 0;
  const int s0 = g * a.spw, ns = deep && min(a.spw, i0 - s0) > 0 ? min(a.spw, i0 - s0) : 0;
  const int top = deep ? L - 1 : 2;   // act[l] / dz[l] exist for l = 2 .. top
  // ---- LDS layout (ae_online_plan counts exactly this) -----------------------------------------------------------------
  S* p = reinterpret_cast<S*>(lds_raw);
  S* W1s = p; p += (long)a.rpw * i0;          // [rpw][i0]
  S* b1s = p; p += a.rpw;
  const int rp2 = a.rpw | 1;                  // W2s' row stride, odd: threads one row apart fall into different LDS banks
  S* W2s = p; p += (long)o2 * rp2;            // [o2][rp2]: columns R_g of W2
  S* b2s = p; p += o2;                        // (replicated)
  S* Wr[AE_ONLINE_MAX_LAYERS];                // replicated layers l + 1 = 3 .. L-1: [o_{l+1}][o_l + 1], rows padded by one
  S* br[AE_ONLINE_MAX_LAYERS];
  for (int l = 2; l + 1 < L; ++l) {
    Wr[l] = p; p += (long)a.dims[l + 1] * (a.dims[l] + 1);
    br[l] = p; p += a.dims[l + 1];
  }
  S *WLs = p, *bLs = p, *dzLs = p;            // rows S_g of layer L: [spw][o_{L-1} + 1]
  if (deep) {
    p += (long)a.spw * (KL + 1);
    bLs = p; p += a.spw;
    dzLs = p; p += a.spw;
  }
  S* xs = p; p += i0;
  S* h1s = p; p += a.rpw;
  S* dz1s = p; p += a.rpw;
  S* act[AE_ONLINE_MAX_LAYERS + 1];           // act[l]: the output of layer l, whole (L = 2: a_2 = the reconstruction)
  S* dz[AE_ONLINE_MAX_LAYERS + 1];
  for (int l = 2; l <= top; ++l) {
    act[l] = p; p += a.dims[l];
    dz[l] = p; p += a.dims[l];
  }
  S* red = p; p += AO_RED;
  // ---- parameters -> LDS ---------------------------------------------------------------------------------------------
  for (long e = tid; e < (long)nr * i0; e += AO_THREADS) W1s[e] = a.W[0][(long)r0 * i0 + e];
  for (int e = tid; e < nr; e += AO_THREADS) b1s[e] = a.b[0][r0 + e];
  for (long e = tid; e < (long)o2 * a.rpw; e += AO_THREADS) {
    const int j = (int)(e / a.rpw), r = (int)(e - (long)j * a.rpw);
    W2s[(long)j * rp2 + r] = r < nr ? a.W[1][(long)j * o1 + r0 + r] : S(0.);
  }
  for (int e = tid; e < o2; e += AO_THREADS) b2s[e] = a.b[1][e];
  for (int l = 2; l + 1 < L; ++l) {
    const int K = a.dims[l], O = a.dims[l + 1];
    for (long e = tid; e < (long)O * K; e += AO_THREADS) Wr[l][(e / K) * (K + 1) + e % K] = a.W[l][e];
    for (int e = tid; e < O; e += AO_THREADS) br[l][e] = a.b[l][e];
  }
  if (deep) {
    for (long e = tid; e < (long)ns * KL; e += AO_THREADS) WLs[(e / KL) * (KL + 1) + e % KL] = a.W[L - 1][(long)s0 * KL + e];
    for (int e = tid; e < ns; e += AO_THREADS) bLs[e] = a.b[L - 1][s0 + e];
  }
  auto row_of = [&](long t) { return a.idx ? (long)a.idx[t] : t; };
  S xr[AO_XREGS];   // the first sample's row
  {
    const long s = row_of(0);
#pragma unroll
    for (int q = 0; q < AO_XREGS; ++q) {
      const int k = tid + q * AO_THREADS;
      xr[q] = k < i0 ? a.X[s * i0 + k] : S(0.);
    }
  }
  long s_next = a.n > 1 ? row_of(1) : 0;  // the row index is fetched one sample further ahead than the row
  if (tid < AO_RED) red[tid] = S(0.);
  __syncthreads();
  const S rate = a.rate;
  constexpr int WORDS = sizeof(S) / 4;
  // the next sample's row is requested behind the LAST wait on memory of a sample: loads return in order, so issued any
  // earlier an exchange would sit behind a row that comes from HBM
  auto prefetch = [&](long t) {
    if (t + 1 < a.n) {
      const long s = s_next;
#pragma unroll
      for (int q = 0; q < AO_XREGS; ++q) {
        const int k = tid + q * AO_THREADS;
        if (k < i0) xr[q] = a.X[s * i0 + k];
      }
      if (t + 2 < a.n) s_next = row_of(t + 2);
    }
  };
  for (long t = 0; t < a.n; ++t) {
#pragma unroll
    for (int q = 0; q < AO_XREGS; ++q) {
      const int k = tid + q * AO_THREADS;
      if (k < i0) xs[k] = xr[q];
    }
    __syncthreads();
    // ---- layer 1, this workgroup's rows: one wave a row ----------------------------------------------------------------
    for (int r = wave; r < nr; r += AO_NW) {
      const S z = dm::wave_dot(W1s + (long)r * i0, xs, i0, lane);
      if (lane == 0) h1s[r] = ao_act(a.kind[0], z + b1s[r]);
    }
    __syncthreads();
    // ---- exchange 1: partial z2 = W2[:, R_g] a1[R_g] out, z2 = b2 + the G partials in workgroup order back -------------
    const unsigned tag = (unsigned)(t + 1);
    bool ok = true;
    S lsum = S(0.);   // L = 2: this thread's part of the squared error
    {
      unsigned long long* ex = a.ex1 + (long)(t & 1) * G * o2 * WORDS;
      for (int j = tid; j < o2; j += AO_THREADS) {
        const S* w = W2s + (long)j * rp2;
        S acc = S(0.);
        for (int r = 0; r < nr; ++r) acc = dm::fma(w[r], h1s[r], acc);
        if (G == 1) act[2][j] = acc;   // (read back by this very thread)
        else xe::publish(ex + ((long)g * o2 + j) * WORDS, acc, tag);
      }
      for (int j = tid; j < o2; j += AO_THREADS) {
        const S s = G == 1 ? act[2][j] : ao_gather<S>(ex, G, o2, j, tag, a.timeout, ok);
        const S h = ao_act(a.kind[1], b2s[j] + s);
        act[2][j] = h;
        if (!deep) {   // layer 2 is the last one: the head, redundantly in every workgroup
          const S d = h - xs[j];
          lsum += d * d;
          dz[2][j] = S(2) * d * ao_dact(a.kind[1], h);
        }
      }
    }
    if (!deep) prefetch(t);
    if (!ok) {
      *a.status = (int)(t + 1);
      red[AO_FLAG] = S(1.);
    }
    if (!deep) {
      lsum = dm::wave_sum(lsum);
      if (lane == 0) red[wave] = lsum;
    }
    __syncthreads();
    if (red[AO_FLAG] != S(0.)) {
      xe::give_up(a.votes, g);   // (a peer never showed up; uniform: read behind a barrier)
      return;
    }
    if (!deep) {
      if (g == 0 && tid == 0 && a.losses) {
        S l = S(0.);
        for (int q = 0; q < AO_NW; ++q) l += red[q];
        a.losses[t] = l;
      }
    } else {
      // ---- replicated layers 3 .. L-1: one wave an output ------------------------------------------------------------------
      for (int l = 2; l + 1 < L; ++l) {
        const int K = a.dims[l], O = a.dims[l + 1];
        for (int j = wave; j < O; j += AO_NW) {
          const S z = dm::wave_dot(Wr[l] + (long)j * (K + 1), act[l], K, lane);
          if (lane == 0) act[l + 1][j] = ao_act(a.kind[l], z + br[l][j]);
        }
        __syncthreads();
      }
      // ---- layer L on rows S_g: z, the head and this workgroup's part of the squared error ------------------------------------
      S lpart = S(0.);   // (lane 0 of a wave: its rows in order)
      for (int r = wave; r < ns; r += AO_NW) {
        const S z = dm::wave_dot(WLs + (long)r * (KL + 1), act[L - 1], KL, lane);
        if (lane == 0) {
          const S h = ao_act(a.kind[L - 1], z + bLs[r]), d = h - xs[s0 + r];
          lpart += d * d;
          dzLs[r] = S(2) * d * ao_dact(a.kind[L - 1], h);
        }
      }
      if (lane == 0) red[wave] = lpart;
      __syncthreads();
      // ---- exchange 2: W_L[S_g, :]^T dz_L[S_g] and the loss partial out, their sums in workgroup order back --------------------
      const int n2 = KL + 1;
      unsigned long long* ex = a.ex2 + (long)(t & 1) * G * n2 * WORDS;
      for (int k = tid; k < n2; k += AO_THREADS) {
        S c = S(0.);
        if (k < KL) {
          for (int r = 0; r < ns; ++r) c = dm::fma(WLs[(long)r * (KL + 1) + k], dzLs[r], c);
        } else {
          for (int q = 0; q < AO_NW; ++q) c += red[q];
        }
        if (G > 1) xe::publish(ex + ((long)g * n2 + k) * WORDS, c, tag);
        else if (k < KL) dz[L - 1][k] = c;
        else red[AO_LOSS] = c;
      }
      for (int k = tid; k < n2; k += AO_THREADS) {
        const S s = G > 1 ? ao_gather<S>(ex, G, n2, k, tag, a.timeout, ok) : k < KL ? dz[L - 1][k] : red[AO_LOSS];
        if (k < KL) dz[L - 1][k] = s * ao_dact(a.kind[L - 2], act[L - 1][k]);
        else if (g == 0 && a.losses) a.losses[t] = s;
      }
      prefetch(t);
      if (!ok) {
        *a.status = (int)(t + 1);
        red[AO_FLAG] = S(1.);
      }
      __syncthreads();
      if (red[AO_FLAG] != S(0.)) {
        xe::give_up(a.votes, g);   // (a peer never showed up; uniform: read behind a barrier)
        return;
      }
      // ---- back through the replicated layers (OLD weights) --------------------------------------------------------------------
      for (int l = L - 2; l >= 2; --l) {
        const int K = a.dims[l], O = a.dims[l + 1];
        for (int k = tid; k < K; k += AO_THREADS) {
          S s = S(0.);
          for (int j = 0; j < O; ++j) s = dm::fma(Wr[l][(long)j * (K + 1) + k], dz[l + 1][j], s);
          dz[l][k] = s * ao_dact(a.kind[l - 1], act[l][k]);
        }
        __syncthreads();
      }
    }
    // ---- dz1 on this workgroup's rows: W2[:, R_g]^T dz2, one wave a row ----------------------------------------------------
    for (int r = wave; r < nr; r += AO_NW) {
      S s = S(0.);
      for (int j = lane; j < o2; j += 64) s = dm::fma(W2s[(long)j * rp2 + r], dz[2][j], s);
      s = dm::wave_sum(s);
      if (lane == 0) dz1s[r] = s * ao_dact(a.kind[0], h1s[r]);
    }
    __syncthreads();
    // ---- p <- p - rate * g, everything this workgroup holds ------------------------------------------------------------------
    // (a thread owns its columns k of W1's rows: the input element is read once, four rows go as a group so that their LDS
    //  round trips overlap)
    for (int k = tid; k < i0; k += AO_THREADS) {
      const S x = -rate * xs[k];
      S* __restrict__ w = W1s + k;
      int r = 0;
      for (; r + 4 <= nr; r += 4) {
        S w0 = w[(long)(r + 0) * i0], w1 = w[(long)(r + 1) * i0], w2 = w[(long)(r + 2) * i0], w3 = w[(long)(r + 3) * i0];
        w0 = dm::fma(dz1s[r + 0], x, w0);
        w1 = dm::fma(dz1s[r + 1], x, w1);
        w2 = dm::fma(dz1s[r + 2], x, w2);
        w3 = dm::fma(dz1s[r + 3], x, w3);
        w[(long)(r + 0) * i0] = w0; w[(long)(r + 1) * i0] = w1; w[(long)(r + 2) * i0] = w2; w[(long)(r + 3) * i0] = w3;
      }
      for (; r < nr; ++r) w[(long)r * i0] = dm::fma(dz1s[r], x, w[(long)r * i0]);
    }
    for (int e = tid; e < nr; e += AO_THREADS) b1s[e] -= rate * dz1s[e];
    for (int j = tid; j < o2; j += AO_THREADS) {
      const S c = -rate * dz[2][j];
      S* __restrict__ w = W2s + (long)j * rp2;
      for (int r = 0; r < nr; ++r) w[r] = dm::fma(c, h1s[r], w[r]);
      b2s[j] += c;
    }
    for (int l = 2; l + 1 < L; ++l) {
      const int K = a.dims[l], O = a.dims[l + 1];
      for (int e = tid; e < O * K; e += AO_THREADS) {
        const int j = e / K, k = e - j * K;
        S* w = Wr[l] + (long)j * (K + 1) + k;
        *w = dm::fma(-rate * dz[l + 1][j], act[l][k], *w);
      }
      for (int e = tid; e < O; e += AO_THREADS) br[l][e] -= rate * dz[l + 1][e];
    }
    if (deep) {
      for (int e = tid; e < ns * KL; e += AO_THREADS) {
        const int r = e / KL, k = e - r * KL;
        S* w = WLs + (long)r * (KL + 1) + k;
        *w = dm::fma(-rate * dzLs[r], act[L - 1][k], *w);
      }
      for (int e = tid; e < ns; e += AO_THREADS) bLs[e] -= rate * dzLs[e];
    }
    __syncthreads();
  }
  // ---- commit: ONE decision for all workgroups --------------------------------------------------------------------------
  // (written out here and in online_sgd.hip: as a function, in each form tried, this file's assembly moves -- xcd_exchange.hpp)
  if (G > 1) {
    if (tid == 0) __hip_atomic_store(a.votes + g, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (tid < G) {
      const long long c0 = wall_clock64();
      unsigned long long v = 0;
      while (true) {
        v = __hip_atomic_load(a.votes + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (v != 0) break;
        if (__hip_atomic_load(a.votes + xe::DECISION, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) break;   // (decided meanwhile)
        if (wall_clock64() - c0 > a.timeout) break;
        __builtin_amdgcn_s_sleep(1);
      }
      if (v != 1ull) red[AO_FLAG] = S(1.);   // (any thread: a vote that is missing or "failed")
    }
    __syncthreads();
    if (tid == 0) {
      unsigned long long expect = 0ull;
      const unsigned long long mine = red[AO_FLAG] != S(0.) ? xe::ABORT : xe::COMMIT;
      const bool won = __hip_atomic_compare_exchange_strong(a.votes + xe::DECISION, &expect, mine, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                            __HIP_MEMORY_SCOPE_AGENT);
      const unsigned long long decision = won ? mine : expect;   // (expect holds what was there)
      red[AO_VERDICT] = decision == xe::COMMIT ? S(1.) : S(0.);
      if (decision == xe::ABORT && *a.status == 0) *a.status = (int)(a.n + 1);   // (no sample to name: reported as "sample n")
    }
    __syncthreads();
    if (red[AO_VERDICT] != S(1.)) return;
  }
  // ---- parameters back to memory (replicated ones from workgroup 0: all copies are the same bits) -----------------------
  for (long e = tid; e < (long)nr * i0; e += AO_THREADS) a.W[0][(long)r0 * i0 + e] = W1s[e];
  for (int e = tid; e < nr; e += AO_THREADS) a.b[0][r0 + e] = b1s[e];
  for (long e = tid; e < (long)o2 * a.rpw; e += AO_THREADS) {
    const int j = (int)(e / a.rpw), r = (int)(e - (long)j * a.rpw);
    if (r < nr) a.W[1][(long)j * o1 + r0 + r] = W2s[(long)j * rp2 + r];
  }
  if (deep) {
    for (long e = tid; e < (long)ns * KL; e += AO_THREADS) a.W[L - 1][(long)s0 * KL + e] = WLs[(e / KL) * (KL + 1) + e % KL];
    for (int e = tid; e < ns; e += AO_THREADS) a.b[L - 1][s0 + e] = bLs[e];
  }
  if (g == 0) {
    for (int e = tid; e < o2; e += AO_THREADS) a.b[1][e] = b2s[e];
    for (int l = 2; l + 1 < L; ++l) {
      const int K = a.dims[l], O = a.dims[l + 1];
      for (long e = tid; e < (long)O * K; e += AO_THREADS) a.W[l][e] = Wr[l][(e / K) * (K + 1) + e % K];
      for (int e = tid; e < O; e += AO_THREADS) a.b[l][e] = br[l][e];
    }
  }
}

xe::XcdExchange g_ao(true);

template <class S>
void launch_ae_online_t(const AeOnlinePlan& plan, int L, const int64_t* dims, const int* kinds, void* const* W, void* const* b,
                        const void* X, const long long* idx_dev, int64_t n, double rate, void* losses, size_t ex1_bytes,
                        hipStream_t s) {
  AeOnlineArgs<S> a{};
  a.L = L;
  for (int l = 0; l <= L; ++l) a.dims[l] = (int)dims[l];
  for (int l = 0; l < L; ++l) {
    a.kind[l] = kinds[l];
    a.W[l] = static_cast<S*>(W[l]);
    a.b[l] = static_cast<S*>(b[l]);
  }
  a.X = static_cast<const S*>(X);
  a.idx = idx_dev;
  a.n = n;
  a.rate = (S)rate;
  a.losses = static_cast<S*>(losses);
  a.G = plan.G;
  a.rpw = plan.rpw;
  a.spw = plan.spw;
  a.ex1 = g_ao.exch();
  a.ex2 = g_ao.exch() + ex1_bytes / 8;
  a.votes = g_ao.votes();
  a.status = g_ao.status_dev<int>();
  a.timeout = xe::watchdog_ticks();
  xe::allow_full_lds<ae_online_kernel<S>>();
  launch_k(ae_online_kernel<S>, dim3((unsigned)plan.grid), dim3(AO_THREADS), plan.lds, s, a);
}

}  // namespace

// The plan: the SMALLEST G (from min_groups on, at most 32) that gives every workgroup at least one row of layer 1 and, for
// L >= 3, of layer L, and whose workgroups fit 160 KiB of LDS.  2..6 layers, i0 <= 2048 = dims[L], every width <= 65535.
bool ae_online_plan(int dtype, int L, const int64_t* dims, int min_groups, AeOnlinePlan* plan) {
  const int64_t es = dtype == TO_F64 ? 8 : 4;
  if (L < 2 || L > AE_ONLINE_MAX_LAYERS) return false;
  for (int l = 0; l <= L; ++l)
    if (dims[l] < 1 || dims[l] > 65535) return false;
  if (dims[0] > AO_THREADS * AO_XREGS || dims[L] != dims[0]) return false;
  const bool deep = L >= 3;
  const int64_t i0 = dims[0], o1 = dims[1], o2 = dims[2], KL = dims[L - 1];
  const int64_t gmax = std::min<int64_t>(32, deep ? std::min(o1, dims[L]) : o1);
  for (int64_t G = std::max(1, min_groups); G <= gmax; ++G) {
    const int64_t rpw = (o1 + G - 1) / G, spw = deep ? (dims[L] + G - 1) / G : 0;
    if ((o1 + rpw - 1) / rpw != G || (deep && (dims[L] + spw - 1) / spw != G)) continue;  // a workgroup without a row
    int64_t f = rpw * i0 + rpw + o2 * (rpw | 1) + o2;
    for (int l = 2; l + 1 < L; ++l) f += dims[l + 1] * (dims[l] + 1) + dims[l + 1];
    if (deep) f += spw * (KL + 1) + 2 * spw;
    f += i0 + 2 * rpw + AO_RED;
    for (int l = 2; l <= (deep ? L - 1 : 2); ++l) f += 2 * dims[l];
    if (f * es > AO_LDS_MAX) continue;
    plan->G = (int)G;
    plan->rpw = (int)rpw;
    plan->spw = (int)spw;
    plan->lds = (size_t)(f * es);
    plan->grid = G == 1 ? 1 : 8 * G;
    return true;
  }
  return false;
}

void launch_ae_online(int dtype, const AeOnlinePlan& plan, int L, const int64_t* dims, const int* kinds, void* const* W,
                      void* const* b, const void* X, const long long* idx_dev, int64_t n, double rate, void* losses,
                      hipStream_t s) {
  TO_CHECK(L >= 2 && L <= AE_ONLINE_MAX_LAYERS && n >= 1 && n <= 2147483647LL, TO_ERR_STATE, "internal: autoencoder online kernel: out of range");
  const size_t words = dtype == TO_F64 ? 2 : 1;
  const size_t ex1 = (size_t)2 * plan.G * dims[2] * words * 8, ex2 = L >= 3 ? (size_t)2 * plan.G * (dims[L - 1] + 1) * words * 8 : 0;
  g_ao.reserve(ex1 + ex2);
  g_ao.status_reset();
  if (plan.G > 1) g_ao.zero(s);
  if (dtype == TO_F64) launch_ae_online_t<double>(plan, L, dims, kinds, W, b, X, idx_dev, n, rate, losses, ex1, s);
  else launch_ae_online_t<float>(plan, L, dims, kinds, W, b, X, idx_dev, n, rate, losses, ex1, s);
  TO_HIP(hipGetLastError());
  count_launch();
}

int ae_online_status() { return g_ao.status<int>() ? *g_ao.status<int>() : 0; }

}  // namespace to
