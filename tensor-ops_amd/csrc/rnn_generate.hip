// Closed-loop generation of a recurrent stack (to_rnn_stack_generate): `runNetworkSt` under `iterate` -- after the prime,
// every step's input is made from the step before's stored output row, so nothing of a step is time-independent and
// stack_rnn.cpp's one-GEMM-over-all-rows forward does not apply.
//   gen_feed       : THE feed rule (a wave per row): the next input row and, in the one-hot modes, the symbol, from the
//                    stored previous output row.  TO_FEED_ARGMAX follows arg_max_rows_kernel (reduce_layout.hip) exactly --
//                    the same per-lane fold and the same xor tree, and with a NaN in the row the same fold again over the
//                    elements behind the last NaN -- so the symbol is bit for bit what to_arg_max returns for the stored row,
//                    ties (earliest index) and NaN included.  TO_FEED_SAMPLE is the inverse CDF of the public
//                    header, every operation sequential and in the row's dtype on one lane.
//   feed_kernel    : route A, one launch a generated step: gen_feed over [B][n] rows in memory.
//   rnn_gen_kernel : route B, ONE launch for the Tp prime steps and all G generated steps.  Like rnn_seq_kernel a workgroup
//                    owns R whole sequences, here with the whole stack: nothing crosses workgroups -- no spin, no residency requirement, any grid size.  LDS
//                    holds every layer's W, W' and b (matrices k-major, M[k][j]: consecutive threads read consecutive
//                    columns, conflict-free), and per row the current input, two ping-pong activation rows and every
//                    stateful layer's state twice.  Rows are `wpad` (odd) elements apart and states n | 1, so the lanes of
//                    a wave that work on different rows read a[r][k] from different banks (one address per row: a
//                    broadcast within the row).  Per step and layer the (row, column) items are spread over the threads;
//                    an item is one dot product in a fixed order, the input part and then the state part; one barrier a
//                    layer.  The head (max-subtracted softmax or logistic, a wave per row) works on the row in LDS, stores
//                    it to out[b][k][:] with coalesced stores and feeds it through gen_feed; the next input never leaves
//                    LDS.  Final states are written once at the end.  A row's bits depend neither on B nor on its place.
// Plain VALU FMAs from LDS (an MFMA form for R >= 16 does not exist yet).
#include <algorithm>

#include "common.hpp"
#include "devmath.hpp"

namespace to {

namespace {

constexpr int GEN_THREADS = 256;
constexpr int64_t GEN_MAX_ITEMS = 4096;      // (row, column) items of the widest layer per workgroup

// The feed rule, by one whole wave (all 64 lanes call it): x[0 .. n) = the input made from row[0 .. n); returns the symbol
// (0 for TO_FEED_OUTPUT) on every lane.  row and x do not overlap.
template <class S>
__device__ __forceinline__ int gen_feed(const S* row, int n, int feed, S u, S* x, int lane) {
  int c = 0;
  if (feed == TO_FEED_ARGMAX) {
    S best = S(0);
    long bi = -1, ln = -1;   // ln: the last NaN this lane met
    for (long j = lane; j < n; j += 64) {
      const S v = row[j];
      if (v != v) ln = j;
      if (bi < 0 || !(best >= v)) { best = v; bi = j; }
    }
    if (__ballot(ln >= 0)) {   // a NaN in the row: the fold again, over the elements behind the last one
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        const long ol = __shfl_xor((long long)ln, off, 64);
        ln = ol > ln ? ol : ln;
      }
      best = S(0);
      bi = -1;
      for (long j = lane; j < n; j += 64) {
        if (j <= ln) continue;
        const S v = row[j];
        if (bi < 0 || !(best >= v)) { best = v; bi = j; }
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const S ob = __shfl_xor(best, off, 64);
      const long oi = __shfl_xor((long long)bi, off, 64);
      if (oi >= 0 && (bi < 0 || (oi < bi ? !(ob < best) : !(best >= ob)))) { best = ob; bi = oi; }
    }
    c = __shfl(bi < 0 ? n - 1 : (int)bi, 0, 64);   // lane 0's winner is the one arg_max_rows_kernel stores
  } else if (feed == TO_FEED_SAMPLE) {
    if (lane == 0) {   // c_0 = p_0, c_j = c_{j-1} + p_j; thr = u * c_{n-1}; the symbol = #{j : c_j <= thr}, at most n - 1
      S tot = row[0];
      for (int j = 1; j < n; ++j) tot = tot + row[j];
      const S thr = u * tot;
      S cj = row[0];
      int cnt = cj <= thr ? 1 : 0;
      for (int j = 1; j < n; ++j) {
        cj = cj + row[j];
        cnt += cj <= thr ? 1 : 0;
      }
      c = cnt < n - 1 ? cnt : n - 1;
    }
    c = __shfl(c, 0, 64);
  }
  if (feed == TO_FEED_OUTPUT)
    for (int j = lane; j < n; j += 64) x[j] = row[j];
  else
    for (int j = lane; j < n; j += 64) x[j] = j == c ? S(1) : S(0);
  return c;
}

template <class S>
__global__ __launch_bounds__(GEN_THREADS) void feed_kernel(const S* __restrict__ prev, long B, int n, int feed,
                                                           const S* __restrict__ U, long G, long k, S* __restrict__ x,
                                                           long long* __restrict__ sym) {
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);   // a wave per row: a wave leaves as a whole
  if (row >= B) return;
  const int lane = threadIdx.x & 63;
  const S u = feed == TO_FEED_SAMPLE ? U[row * G + k] : S(0);
  const int c = gen_feed(prev + row * n, n, feed, u, x + row * n, lane);
  if (lane == 0 && sym) sym[row * G + k] = c;
}

template <class S>
struct RnnGenArgs {
  const S* W[RNN_GEN_MAX_LAYERS];      // [n_l][n_{l-1}]
  const S* WS[RNN_GEN_MAX_LAYERS];     // [n_l][n_l] (stateful)
  const S* b[RNN_GEN_MAX_LAYERS];
  const S* s_in[RNN_GEN_MAX_LAYERS];   // the initial states: element (b, j) at b * s_sb[l] + j * s_ss[l]
  long s_sb[RNN_GEN_MAX_LAYERS], s_ss[RNN_GEN_MAX_LAYERS];
  S* s_out[RNN_GEN_MAX_LAYERS];        // [B][n_l] or null
  int n[RNN_GEN_MAX_LAYERS + 1];
  int sk[RNN_GEN_MAX_LAYERS];          // state activation, -1: stateless
  const S* X;                          // the prime: element (b, t, j) at b * x_sb + t * x_st + j * x_sj
  long x_sb, x_st, x_sj;
  S* prime_out;                        // [B][Tp][n_L] or null
  const S* U;                          // [B][G]
  S* out;                              // [B][G][n_L]
  long long* sym;                      // [B][G]
  long B, Tp, G;
  int L, R, wpad, hidden_kind, softmax, feed;
};

template <class S>
__global__ __launch_bounds__(GEN_THREADS) void rnn_gen_kernel(RnnGenArgs<S> a) {
  extern __shared__ __align__(16) unsigned char gen_lds[];
  S* const par = reinterpret_cast<S*>(gen_lds);
  const int L = a.L, R = a.R, wp = a.wpad, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nL = a.n[L];
  const long b0 = (long)blockIdx.x * R;
  const int rows = (int)min((long)R, a.B - b0);
  // ---- the parameters, once: per layer Wk [m][n], WSk [n][n] (stateful), b [n] ------------------------------------------
  S* q = par;
  for (int l = 0; l < L; ++l) {
    const int m = a.n[l], n = a.n[l + 1];
    const S* W = a.W[l];
    for (int e = tid; e < n * m; e += GEN_THREADS) {
      const int j = e / m, k = e - j * m;
      q[k * n + j] = W[e];
    }
    q += n * m;
    if (a.sk[l] >= 0) {
      const S* WS = a.WS[l];
      for (int e = tid; e < n * n; e += GEN_THREADS) {
        const int j = e / n, k = e - j * n;
        q[k * n + j] = WS[e];
      }
      q += n * n;
    }
    const S* bb = a.b[l];
    for (int e = tid; e < n; e += GEN_THREADS) q[e] = bb[e];
    q += n;
  }
  S* const xin = q;                           // [R][wp]: the current input
  S* const act0 = xin + (size_t)R * wp;       // [R][wp] twice: the layers' outputs, ping-pong
  S* const act1 = act0 + (size_t)R * wp;
  S* const sbase = act1 + (size_t)R * wp;     // per stateful layer [2][R][n | 1]
  {
    S* sq = sbase;
    for (int l = 0; l < L; ++l) {
      if (a.sk[l] < 0) continue;
      const int n = a.n[l + 1], sp = n | 1;
      const S* si = a.s_in[l];
      const long sb = a.s_sb[l], ss = a.s_ss[l];
      for (int e = tid; e < rows * n; e += GEN_THREADS) {
        const int r = e / n, j = e - r * n;
        sq[r * sp + j] = si[(b0 + r) * sb + j * ss];
      }
      sq += 2 * (size_t)R * sp;
    }
  }
  const S* fed_from = nullptr;   // the last step's output rows in LDS
  const int n0 = a.n[0];
  for (long t = 0; t < a.Tp + a.G; ++t) {
    const long k = t - a.Tp;   // the generated step (< 0: a prime step)
    if (k < 0) {
      // ---- prime: the step's rows of X ---------------------------------------------------------------------------------
      for (int e = tid; e < rows * n0; e += GEN_THREADS) {
        const int r = e / n0, j = e - r * n0;
        xin[(size_t)r * wp + j] = a.X[(b0 + r) * a.x_sb + t * a.x_st + j * a.x_sj];
      }
    } else {
      // ---- feed: a wave per row ----------------------------------------------------------------------------------------
      for (int r = wave; r < rows; r += GEN_THREADS / 64) {
        const long gr = b0 + r;
        const S u = a.feed == TO_FEED_SAMPLE ? a.U[gr * a.G + k] : S(0);
        const int c = gen_feed(fed_from + (size_t)r * wp, nL, a.feed, u, xin + (size_t)r * wp, lane);
        if (lane == 0 && a.sym) a.sym[gr * a.G + k] = c;
      }
    }
    __syncthreads();
    // ---- the stack: z = W a + W' s + b, new state state_act(z), output hidden_act(z) (the last layer: z, for the head) --------
    const int cs = (int)(t & 1);
    const S* in = xin;
    S* outb = act0;
    const S* pq = par;
    S* sq = sbase;
    for (int l = 0; l < L; ++l) {
      const int m = a.n[l], n = a.n[l + 1], sk = a.sk[l];
      const bool last = l + 1 == L;
      const S* Wk = pq;
      pq += n * m;
      const S* WSk = pq;
      if (sk >= 0) pq += n * n;
      const S* bb = pq;
      pq += n;
      const int sp = n | 1;
      const S* sc = sq + (size_t)cs * R * sp;
      S* sn = sq + (size_t)(cs ^ 1) * R * sp;
      for (int item = tid; item < rows * n; item += GEN_THREADS) {
        const int r = item / n, j = item - r * n;
        const S* ar = in + (size_t)r * wp;
        const S* wj = Wk + j;
        S acc = S(0);
#pragma unroll 4
        for (int kk = 0; kk < m; ++kk) acc = dm::fma(ar[kk], wj[(size_t)kk * n], acc);
        if (sk >= 0) {
          const S* sr = sc + (size_t)r * sp;
          const S* vj = WSk + j;
#pragma unroll 4
          for (int kk = 0; kk < n; ++kk) acc = dm::fma(sr[kk], vj[(size_t)kk * n], acc);
        }
        const S z = acc + bb[j];
        if (sk >= 0) sn[(size_t)r * sp + j] = dm::act(sk, z);
        outb[(size_t)r * wp + j] = last ? z : dm::act(a.hidden_kind, z);
      }
      if (sk >= 0) sq += 2 * (size_t)R * sp;
      __syncthreads();
      in = outb;
      outb = outb == act0 ? act1 : act0;
    }
    // ---- the head on the row in LDS, a wave per row: in place, and out[b][k][:] ------------------------------------------------
    S* zl = const_cast<S*>(in);
    for (int r = wave; r < rows; r += GEN_THREADS / 64) {
      S* zr = zl + (size_t)r * wp;
      S mx = S(-INFINITY), se = S(0);
      if (a.softmax) {
        for (int j = lane; j < nL; j += 64) mx = dm::max(mx, zr[j]);
        mx = dm::wave_max(mx);
        for (int j = lane; j < nL; j += 64) se += dm::exp(zr[j] - mx);
        se = dm::wave_sum(se);
      }
      S* o = k >= 0 ? a.out + ((b0 + r) * a.G + k) * nL : a.prime_out ? a.prime_out + ((b0 + r) * a.Tp + t) * nL : nullptr;
      for (int j = lane; j < nL; j += 64) {
        const S v = zr[j];
        const S p = a.softmax ? dm::exp(v - mx) / se : dm::logistic(v);
        zr[j] = p;
        if (o) o[j] = p;
      }
    }
    __syncthreads();
    fed_from = zl;
  }
  // ---- the final states ---------------------------------------------------------------------------------------------------
  {
    const int cs = (int)((a.Tp + a.G) & 1);
    const S* sq = sbase;
    for (int l = 0; l < L; ++l) {
      if (a.sk[l] < 0) continue;
      const int n = a.n[l + 1], sp = n | 1;
      if (a.s_out[l]) {
        S* so = a.s_out[l] + b0 * n;
        const S* sc = sq + (size_t)cs * R * sp;
        for (int e = tid; e < rows * n; e += GEN_THREADS) {
          const int r = e / n, j = e - r * n;
          so[e] = sc[r * sp + j];
        }
      }
      sq += 2 * (size_t)R * sp;
    }
  }
}

// elements of LDS: the parameters, and what one row needs
void gen_lds_elems(int L, const int64_t* w, const int* stateful, int64_t* params, int64_t* per_row, int64_t* wpad,
                   int64_t* nmax) {
  int64_t P = 0, S2 = 0, wm = w[0], nm = 1;
  for (int l = 0; l < L; ++l) {
    const int64_t m = w[l], n = w[l + 1];
    P += n * m + n + (stateful[l] ? n * n : 0);
    if (stateful[l]) S2 += 2 * (n | 1);
    wm = std::max(wm, n);
    nm = std::max(nm, n);
  }
  *params = P;
  *wpad = wm | 1;
  *per_row = 3 * (wm | 1) + S2;
  *nmax = nm;
}

template <class S>
void go_gen(const RnnGenPlan& p, const RnnGenOperands& o, hipStream_t s) {
  static bool attr = false;
  if (!attr) {
    TO_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(rnn_gen_kernel<S>), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)GEN_LDS_MAX));
    attr = true;
  }
  RnnGenArgs<S> a{};
  for (int l = 0; l < o.L; ++l) {
    a.W[l] = (const S*)o.W[l]; a.WS[l] = (const S*)o.WS[l]; a.b[l] = (const S*)o.b[l];
    a.s_in[l] = (const S*)o.s_in[l]; a.s_out[l] = (S*)o.s_out[l];
    a.s_sb[l] = (long)o.s_sb[l]; a.s_ss[l] = (long)o.s_ss[l];
    a.sk[l] = o.state_kind[l];
  }
  for (int l = 0; l <= o.L; ++l) a.n[l] = (int)o.widths[l];
  a.X = (const S*)o.X; a.x_sb = (long)o.x_sb; a.x_st = (long)o.x_st; a.x_sj = (long)o.x_sj;
  a.prime_out = (S*)o.prime_out;
  a.U = (const S*)o.U; a.out = (S*)o.out; a.sym = o.sym;
  a.B = (long)o.B; a.Tp = (long)o.Tp; a.G = (long)o.G;
  a.L = o.L; a.R = p.R; a.wpad = p.wpad; a.hidden_kind = o.hidden_kind; a.softmax = o.softmax ? 1 : 0; a.feed = o.feed;
  launch_k(rnn_gen_kernel<S>, dim3((unsigned)p.grid), dim3(GEN_THREADS), p.lds, s, a);
}

}  // namespace

// R rows per workgroup as rnn_seq_plan chooses them -- enough rows to give every thread an item of the widest layer, more
// when the batch would need more than 256 workgroups -- but no more than a row a wave while the batch does not need it: the
// head and the feed take a wave a row, a chain of cross-lane steps that the rows of one wave go through one after the other
// (measured: 5 -> 7 -> 5 at B = 32 was 20 us a step at R = 32 against 4.5 at one row a wave).  Then fewer until the parameters
// and R rows fit the LDS.
bool rnn_gen_plan(int dtype, int L, const int64_t* widths, const int* stateful, int64_t B, RnnGenPlan* p) {
  if (L < 1 || L > RNN_GEN_MAX_LAYERS || B < 1) return false;
  for (int l = 0; l <= L; ++l)
    if (widths[l] < 1 || widths[l] > 65536) return false;
  const int64_t es = dtype == TO_F64 ? 8 : 4;
  int64_t P, per_row, wpad, nmax;
  gen_lds_elems(L, widths, stateful, &P, &per_row, &wpad, &nmax);
  if (P * es > (int64_t)GEN_LDS_MAX) return false;
  const int64_t R_item = std::min<int64_t>(std::max<int64_t>(1, GEN_THREADS / nmax), GEN_THREADS / 64);
  int64_t R = std::max(R_item, (B + 255) / 256);
  R = std::min({R, std::max<int64_t>(1, GEN_MAX_ITEMS / nmax), B});
  const int64_t fit = ((int64_t)GEN_LDS_MAX / es - P) / per_row;
  R = std::min(R, fit);
  if (R < 1) return false;
  p->R = (int)R;
  p->wpad = (int)wpad;
  p->grid = (B + R - 1) / R;
  p->lds = (size_t)((P + R * per_row) * es);
  p->few_items = (R * nmax + GEN_THREADS - 1) / GEN_THREADS <= 4 && p->grid <= 256;
  return p->grid <= 2147483647LL;
}

void launch_rnn_gen(int dtype, const RnnGenPlan& p, const RnnGenOperands& o, hipStream_t s) {
  if (o.B == 0 || o.G == 0) return;
  TO_CHECK(o.L >= 1 && o.L <= RNN_GEN_MAX_LAYERS && p.R >= 1 && p.lds <= GEN_LDS_MAX, TO_ERR_STATE,
           "internal: rnn_gen outside its plan");
  if (dtype == TO_F64) go_gen<double>(p, o, s);
  else go_gen<float>(p, o, s);
  TO_HIP(hipGetLastError());
  count_launch();
}

void launch_rnn_feed(int dtype, const void* prev, int64_t B, int64_t n, int feed, const void* U, int64_t G, int64_t k, void* x,
                     long long* sym, hipStream_t s) {
  if (B == 0) return;
  const dim3 grid((unsigned)((B + 3) / 4));
  if (dtype == TO_F64)
    launch_k(feed_kernel<double>, grid, dim3(GEN_THREADS), 0, s, (const double*)prev, (long)B, (int)n, feed,
             (const double*)U, (long)G, (long)k, (double*)x, sym);
  else
    launch_k(feed_kernel<float>, grid, dim3(GEN_THREADS), 0, s, (const float*)prev, (long)B, (int)n, feed, (const float*)U,
             (long)G, (long)k, (float*)x, sym);
  TO_HIP(hipGetLastError());
  count_launch();
}

}  // namespace to
