// `induceNetwork` iterated (FeedForward.hs:150-164; app/MNIST.hs:357-365 runs it 5000 times in a row): gradient descent on
// the INPUT of an ffLayer stack with the parameters fixed, ALL iterations of a row in ONE persistent launch.
//
//   x_{k+1} = x_k - rate * d/dx loss(net(x_k), y)
//
// is a chain of tiny dependent matrix-vector products in which only the i0 numbers of x change.  The per-iteration route
// (stack_ff.cpp, route A) pays about eight launches an iteration; here the parameters sit in LDS for the whole launch:
//
//   * layer 1 is split by COLUMNS over G <= 32 workgroups of one XCD: workgroup g owns the columns J_g of W_1 (all o1 rows)
//     and the matching slice x[J_g].  The slice never leaves its workgroup: x[J_g] -= rate * W_1[:, J_g]^T dz_1 is local;
//   * forward: every workgroup puts its partial product W_1[:, J_g] x[J_g] (o1 numbers) into an exchange buffer and then
//     sums the G partials in workgroup order (every workgroup gets the same bits): z_1.  ONE exchange per iteration;
//   * layers 2..L, the head, the loss and the cotangents back to dz_1 are replicated in every workgroup; the hidden
//     activation is a template parameter of the kernel: logistic (h (1 - h) backward) or tanh (1 - h h; devmath.hpp);
//   * G == 1 (the stack fits one workgroup's LDS) is the same kernel without any exchange: independent workgroups, as many
//     as there are rows (up to 256), each walking its share of the rows.  With G > 1 one group -- the workgroups with
//     blockIdx.x % 8 == 0 of a grid of 8 G, the others leave at once -- takes the rows one after the other.
//
// The exchange is online_sgd.hip's: {tag, 32 bits of the value} in one 64-bit word, L1-bypassing agent-scope stores and
// loads, two buffers by step parity, and it carries that kernel's precondition -- it is only right between workgroups that
// share one XCD's L2, so a plan with G > 1 may only be launched where online_sgd_placement_ok() holds (the caller asks).
// Every wait is bounded by a wall_clock64 watchdog; a workgroup that gives up reports (iteration, row) in a host-visible
// word and leaves.  The kernel writes only scratch: the host copies to the caller's tensors after a launch that reported
// success.  Residency of the G workgroups comes from the grid size alone (8 G <= 256 workgroups, one per CU).
//
// Range: 1..6 layers, a head of at most 64 outputs, every width <= 65535, everything a workgroup holds within 160 KiB of
// LDS (the plan picks the smallest G that fits): fp32 784-300-100-10 at G = 32 (about 161.6 KB), 784-32-10 at G = 1;
// fp64 784-32-10 at G = 2; fp64 784-300-100-10 does NOT fit (W_2 alone is 240 KB): route A.
// Every sum runs in an order fixed by the plan (dtype and widths only), so a row's bits depend neither on the batch nor on
// the row's place in it, and iters = a followed by iters = b equals iters = a + b.
// The automatic rule (which shapes take this route by default) is in stack_ff.cpp beside the measurements it was derived from
// (tools/induce_scan.py, profiles/r08_induce_scan.txt).
#include "common.hpp"
#include "devmath.hpp"

namespace to {

namespace {

constexpr int IN_THREADS = 512;
constexpr int IN_NWV = IN_THREADS / 64;

template <class S>
struct InduceArgs {
  int L;
  int dims[INDUCE_MAX_LAYERS + 1];  // i0, o1 .. oL
  const S* W[INDUCE_MAX_LAYERS];
  const S* b[INDUCE_MAX_LAYERS];
  S* X;              // [B][i0] contiguous scratch: x_0 on entry, x_iters on exit
  const S* Y;        // rows y_sm apart (0: one target for every row)
  long y_sm;
  S* gx;             // [B][i0] or null: the last iteration's gradient
  S* losses;         // [B][iters] or null
  long B, iters;
  S rate;
  int head;          // 1: softmax >>> crossEntropy, 2: logistic >>> squaredError
  int G, cw;         // workgroups of the group, columns of layer 1 per workgroup
  unsigned long long* exch;  // [2][G][o1][words of S]: {tag, 32 bits of the value} (zero at launch; G > 1 only)
  long long* status; // host-visible: [0] nonzero = a wait timed out at that iteration + 1, [1] its row
  long long timeout; // wall_clock64 ticks
};

// out(j) = sum_k W[j * ld + k] x[k], j < O.  K >= 64: one wave per row, four chains per lane; else one thread per row
// (ld is odd: the rows of consecutive threads start in different banks).  No barrier inside.
template <class S, class F>
__device__ __forceinline__ void matvec(const S* __restrict__ W, int ld, int O, int K, const S* __restrict__ x, F&& put) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (K >= 64) {
    for (int j = wave; j < O; j += IN_NWV) {
      const S* __restrict__ w = W + (long)j * ld;
      S a0 = S(0.), a1 = S(0.), a2 = S(0.), a3 = S(0.);
      int k = lane;
      for (; k + 192 < K; k += 256) {
        a0 = dm::fma(w[k], x[k], a0);
        a1 = dm::fma(w[k + 64], x[k + 64], a1);
        a2 = dm::fma(w[k + 128], x[k + 128], a2);
        a3 = dm::fma(w[k + 192], x[k + 192], a3);
      }
      for (; k < K; k += 64) a0 = dm::fma(w[k], x[k], a0);
      const S acc = dm::wave_sum((a0 + a1) + (a2 + a3));
      if (lane == 0) put(j, acc);
    }
  } else {
    for (int j = tid; j < O; j += IN_THREADS) {
      const S* __restrict__ w = W + (long)j * ld;
      S acc = S(0.);
      for (int k = 0; k < K; ++k) acc = dm::fma(w[k], x[k], acc);
      put(j, acc);
    }
  }
}

// out(k) = sum_j W[j * ld + k] d[j], k < K.  K <= IN_THREADS: the rows are cut into nch = min(IN_THREADS / K, 16, O) runs,
// thread (q, k) sums run q of column k into scr[q * K + k], then thread k adds the runs in order (one barrier inside,
// reached by every thread: nch depends on O and K only).  Wider: one thread per column, all rows.
template <class S, class F>
__device__ __forceinline__ void matvec_t(const S* __restrict__ W, int ld, int O, int K, const S* __restrict__ d, S* scr, F&& put) {
  const int tid = threadIdx.x;
  int nch = K <= IN_THREADS ? IN_THREADS / K : 1;
  nch = nch > 16 ? 16 : nch;
  nch = nch > O ? O : nch;
  if (nch <= 1) {
    for (int k = tid; k < K; k += IN_THREADS) {
      S s = S(0.);
      for (int j = 0; j < O; ++j) s = dm::fma(W[(long)j * ld + k], d[j], s);
      put(k, s);
    }
    return;
  }
  const int len = (O + nch - 1) / nch;
  if (tid < nch * K) {
    const int q = tid / K, k = tid - q * K;
    const int j1 = (q + 1) * len < O ? (q + 1) * len : O;
    S s = S(0.);
    for (int j = q * len; j < j1; ++j) s = dm::fma(W[(long)j * ld + k], d[j], s);
    scr[q * K + k] = s;
  }
  __syncthreads();
  if (tid < K) {
    S s = scr[tid];
    for (int q = 1; q < nch; ++q) s += scr[q * K + tid];
    put(tid, s);
  }
}

template <class S, int ACT>
__global__ __launch_bounds__(IN_THREADS) void induce_seq_kernel(InduceArgs<S> a) {
  int g = 0;
  long grp = blockIdx.x, ngrp = gridDim.x;
  if (a.G > 1) {
    if (blockIdx.x & 7) return;  // one XCD only
    g = blockIdx.x >> 3;
    grp = 0;
    ngrp = 1;
  }
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  S* p = reinterpret_cast<S*>(lds_raw);
  const int L = a.L, i0 = a.dims[0], o1 = a.dims[1], oL = a.dims[L];
  const int c0 = g * a.cw, nc = min(a.cw, i0 - c0) > 0 ? min(a.cw, i0 - c0) : 0;
  // ---- LDS layout (induce_seq_plan counts the same items) -------------------------------------------------------------------
  S* Wl[INDUCE_MAX_LAYERS];
  S* bb[INDUCE_MAX_LAYERS];
  int ld[INDUCE_MAX_LAYERS];
  ld[0] = a.cw | 1;
  Wl[0] = p; p += (long)o1 * ld[0];                    // [o1][cw]: columns J_g of W_1
  for (int l = 1; l < L; ++l) {
    ld[l] = a.dims[l] | 1;
    Wl[l] = p; p += (long)a.dims[l + 1] * ld[l];       // replicated, rows padded to an odd length
  }
  for (int l = 0; l < L; ++l) { bb[l] = p; p += a.dims[l + 1]; }
  S* xs = p; p += a.cw;
  S* ys = p; p += oL;
  S* act[INDUCE_MAX_LAYERS + 1];
  S* dz[INDUCE_MAX_LAYERS + 1];
  for (int l = 1; l <= L; ++l) {
    act[l] = p; p += a.dims[l];
    dz[l] = p; p += a.dims[l];
  }
  S* scr = p; p += IN_THREADS;
  S* red = p; p += 8;
  // ---- parameters -> LDS --------------------------------------------------------------------------------------------------
  for (long e = tid; e < (long)o1 * nc; e += IN_THREADS) {
    const int j = (int)(e / nc), c = (int)(e - (long)j * nc);
    Wl[0][(long)j * ld[0] + c] = a.W[0][(long)j * i0 + c0 + c];
  }
  for (int l = 1; l < L; ++l) {
    const int K = a.dims[l], O = a.dims[l + 1];
    for (long e = tid; e < (long)O * K; e += IN_THREADS) {
      const int j = (int)(e / K), k = (int)(e - (long)j * K);
      Wl[l][(long)j * ld[l] + k] = a.W[l][e];
    }
  }
  for (int l = 0; l < L; ++l)
    for (int e = tid; e < a.dims[l + 1]; e += IN_THREADS) bb[l][e] = a.b[l][e];
  if (tid == 0) red[7] = S(0.);
  __syncthreads();
  const S rate = a.rate;
  constexpr int WORDS = sizeof(S) / 4;
  long step = 0;   // the group's iterations so far, over all of its rows: the exchange's tag and buffer parity
  for (long row = grp; row < a.B; row += ngrp) {
    for (int c = tid; c < nc; c += IN_THREADS) xs[c] = a.X[row * i0 + c0 + c];
    for (int j = tid; j < oL; j += IN_THREADS) ys[j] = a.Y[row * a.y_sm + j];
    __syncthreads();
    for (long k = 0; k < a.iters; ++k, ++step) {
      // ---- layer 1: this workgroup's partial product, then (G > 1) the exchange ----------------------------------------------
      matvec(Wl[0], ld[0], o1, nc, xs, [&](int j, S v) { act[1][j] = v; });
      __syncthreads();
      {
        const unsigned tag = (unsigned)(step + 1);
        unsigned long long* ex = a.exch + (step & 1) * (long)a.G * o1 * WORDS;
        bool ok = true;
        for (int j = tid; j < o1; j += IN_THREADS) {
          S z = act[1][j];
          if (a.G > 1) {
            unsigned wd[WORDS];
            __builtin_memcpy(wd, &z, sizeof(S));
#pragma unroll
            for (int u = 0; u < WORDS; ++u)
              __hip_atomic_store(ex + ((long)g * o1 + j) * WORDS + u, ((unsigned long long)tag << 32) | wd[u], __ATOMIC_RELAXED,
                                 __HIP_MEMORY_SCOPE_AGENT);
            // every partial (this workgroup's too) comes back from L2, eight workgroups' words in flight at a time, and is
            // added in workgroup order
            z = S(0.);
            for (int q0 = 0; q0 < a.G && ok; q0 += 8) {
              const int nq = a.G - q0 < 8 ? a.G - q0 : 8;
              unsigned long long v[8 * WORDS];
              unsigned pend = (1u << (nq * WORDS)) - 1u;
              const long long t0 = wall_clock64();
              while (true) {
#pragma unroll
                for (int u = 0; u < 8 * WORDS; ++u)
                  if ((pend >> u) & 1u)
                    v[u] = __hip_atomic_load(ex + ((long)(q0 + u / WORDS) * o1 + j) * WORDS + (u % WORDS), __ATOMIC_RELAXED,
                                             __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
                for (int u = 0; u < 8 * WORDS; ++u)
                  if (((pend >> u) & 1u) && (unsigned)(v[u] >> 32) == tag) pend &= ~(1u << u);
                if (!pend) break;
                if (wall_clock64() - t0 > a.timeout) {
                  ok = false;
                  break;
                }
                __builtin_amdgcn_s_sleep(1);
              }
              if (ok) {
#pragma unroll
                for (int u = 0; u < 8; ++u)
                  if (u < nq) {
                    unsigned w2[WORDS];
#pragma unroll
                    for (int t = 0; t < WORDS; ++t) w2[t] = (unsigned)v[u * WORDS + t];
                    S part;
                    __builtin_memcpy(&part, w2, sizeof(S));
                    z += part;
                  }
              }
            }
          }
          z += bb[0][j];
          act[1][j] = L == 1 ? z : dm::hid_act_fast<ACT>(z);
        }
        if (!ok) {
          a.status[1] = row;
          a.status[0] = k + 1;
          red[7] = S(1.);   // (any thread: cleared before the loops and only ever set)
        }
      }
      __syncthreads();
      if (red[7] != S(0.)) return;   // a peer never showed up (uniform): nothing is committed, the host sees the status
      // ---- replicated layers 2..L ------------------------------------------------------------------------------------------
      for (int l = 1; l < L; ++l) {
        const bool last = l + 1 == L;
        matvec(Wl[l], ld[l], a.dims[l + 1], a.dims[l], act[l], [&](int j, S v) {
          const S z = v + bb[l][j];
          act[l + 1][j] = last ? z : dm::hid_act_fast<ACT>(z);
        });
        __syncthreads();
      }
      // ---- loss head on z_L (oL <= 64: wave 0) -----------------------------------------------------------------------------
      if (wave == 0) {
        const S z = lane < oL ? act[L][lane] : S(-3.0e38), y = lane < oL ? ys[lane] : S(0.);
        S d, lossv;
        if (a.head == 1) {
          S mx = z;
#pragma unroll
          for (int off = 32; off > 0; off >>= 1) {
            const S other = __shfl_xor(mx, off);
            mx = mx > other ? mx : other;
          }
          const S sy = dm::wave_sum(y);
          const S e = lane < oL ? dm::exp_fast(z - mx) : S(0.);
          const S se = dm::wave_sum(e);
          d = e / se * sy - y;                                      // softmax(z) * sum(y) - y
          lossv = lane < oL ? dm::ce_term(y, z - mx, dm::log(se)) : S(0.);   // -y log softmax(z)
        } else {
          const S s = dm::logistic_fast(z), e = y - s;
          d = -S(2.0) * e * s * (S(1.0) - s);                       // logistic >>> squaredError
          lossv = lane < oL ? e * e : S(0.);
        }
        if (lane < oL) dz[L][lane] = d;
        if (a.losses && g == 0) {
          lossv = dm::wave_sum(lossv);
          if (lane == 0) a.losses[row * a.iters + k] = lossv;
        }
      }
      __syncthreads();
      // ---- cotangents back through the replicated layers ----------------------------------------------------------------------
      for (int l = L - 1; l >= 1; --l) {
        matvec_t(Wl[l], ld[l], a.dims[l + 1], a.dims[l], dz[l + 1], scr, [&](int kk, S s) {
          const S h = act[l][kk];
          dz[l][kk] = dm::hid_dact_fast<ACT>(s, h);
        });
        __syncthreads();
      }
      // ---- this workgroup's slice of the gradient and of the step ------------------------------------------------------------
      const bool want_g = a.gx && k + 1 == a.iters;
      matvec_t(Wl[0], ld[0], o1, nc, dz[1], scr, [&](int c, S s) {
        if (want_g) a.gx[row * i0 + c0 + c] = s;
        xs[c] = xs[c] - rate * s;
      });
      __syncthreads();
    }
    for (int c = tid; c < nc; c += IN_THREADS) a.X[row * i0 + c0 + c] = xs[c];
    __syncthreads();
  }
}

struct InduceState {
  void* exch = nullptr;
  size_t exch_bytes = 0;
  long long* status = nullptr;
  long long* status_dev = nullptr;
};
InduceState g_in;

template <class S, int ACT>
void launch_induce_t(const InduceSeqPlan& plan, int L, const int64_t* dims, const void* const* W, const void* const* b, void* X,
                     const void* Y, int64_t y_sm, void* gx, void* losses, int64_t B, int64_t iters, double rate, int head,
                     hipStream_t s) {
  InduceArgs<S> a{};
  a.L = L;
  for (int l = 0; l <= L; ++l) a.dims[l] = (int)dims[l];
  for (int l = 0; l < L; ++l) {
    a.W[l] = static_cast<const S*>(W[l]);
    a.b[l] = static_cast<const S*>(b[l]);
  }
  a.X = static_cast<S*>(X);
  a.Y = static_cast<const S*>(Y);
  a.y_sm = y_sm;
  a.gx = static_cast<S*>(gx);
  a.losses = static_cast<S*>(losses);
  a.B = B;
  a.iters = iters;
  a.rate = (S)rate;
  a.head = head;
  a.G = plan.G;
  a.cw = plan.cw;
  a.exch = static_cast<unsigned long long*>(g_in.exch);
  a.status = g_in.status_dev;
  static const double timeout_s = [] { const char* e = getenv("TOPS_ONLINE_TIMEOUT_S"); return e ? atof(e) : 2.0; }();
  a.timeout = (long long)(timeout_s * 100e6);
  static bool attr = false;
  if (!attr) {
    TO_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(induce_seq_kernel<S, ACT>), hipFuncAttributeMaxDynamicSharedMemorySize,
                               160 * 1024));
    attr = true;
  }
  launch_k(induce_seq_kernel<S, ACT>, dim3((unsigned)plan.grid), dim3(IN_THREADS), plan.lds, s, a);
}

}  // namespace

// Can the persistent kernel take this stack, and how?  The smallest G whose workgroups hold their share in 160 KiB.
// (G > 1: one group walks all rows, and a tag names one of its iterations -- B * iters must stay below 2^32 - 1.)
bool induce_seq_plan(int dtype, int L, const int64_t* dims, int64_t B, int64_t iters, InduceSeqPlan* plan) {
  const int64_t es = dtype == TO_F64 ? 8 : 4;
  if (L < 1 || L > INDUCE_MAX_LAYERS || B < 1 || iters < 1) return false;
  for (int l = 0; l <= L; ++l)
    if (dims[l] < 1 || dims[l] > 65535) return false;
  if (dims[L] > 64) return false;
  int64_t rest = 0;   // everything but layer 1's slice and x's
  for (int l = 1; l < L; ++l) rest += dims[l + 1] * (dims[l] | 1);
  for (int l = 1; l <= L; ++l) rest += 3 * dims[l];   // bias, activation, cotangent
  rest += dims[L] + IN_THREADS + 8;
  for (int G = 1; G <= (int)std::min<int64_t>(32, dims[0]); ++G) {
    const int64_t cw = (dims[0] + G - 1) / G;
    if ((dims[0] + cw - 1) / cw != G) continue;  // every workgroup owns at least one column
    const int64_t f = dims[1] * (cw | 1) + cw + rest;
    if (f * es > 160 * 1024) continue;
    if (G > 1 && (B > 4000000000LL / iters)) return false;
    plan->G = G;
    plan->cw = (int)cw;
    plan->lds = (size_t)(f * es);
    plan->grid = G > 1 ? 8 * G : std::min<int64_t>(B, 256);
    return true;
  }
  return false;
}

void launch_induce_seq(int dtype, const InduceSeqPlan& plan, int L, const int64_t* dims, const void* const* W,
                       const void* const* b, void* X, const void* Y, int64_t y_sm, void* gx, void* losses, int64_t B,
                       int64_t iters, double rate, int head, int act_kind, hipStream_t s) {
  TO_CHECK(act_kind == ACT_KIND_LOGISTIC || act_kind == ACT_KIND_TANH, TO_ERR_ARG, "induce kernel: unknown hidden activation");
  TO_CHECK(plan.G >= 1 && plan.G <= 32 && plan.grid >= 1 && plan.grid <= 256 && plan.lds <= 160 * 1024, TO_ERR_STATE,
           "induce kernel: not a plan of induce_seq_plan");
  if (!g_in.status) {
    TO_HIP(hipHostMalloc(&g_in.status, 2 * sizeof(long long), hipHostMallocMapped));
    TO_HIP(hipHostGetDevicePointer(reinterpret_cast<void**>(&g_in.status_dev), g_in.status, 0));
  }
  g_in.status[0] = g_in.status[1] = 0;
  if (plan.G > 1) {
    const size_t need = (size_t)2 * plan.G * dims[1] * (dtype == TO_F64 ? 2 : 1) * 8;
    if (g_in.exch_bytes < need) {
      if (g_in.exch) (void)hipFree(g_in.exch);
      g_in.exch = nullptr;
      g_in.exch_bytes = 0;
      TO_HIP(hipMalloc(&g_in.exch, need));
      g_in.exch_bytes = need;
    }
    TO_HIP(hipMemsetAsync(g_in.exch, 0, need, s));  // (no tag of an earlier launch may pass for one of this launch)
  }
  if (act_kind == ACT_KIND_TANH) {
    if (dtype == TO_F64) launch_induce_t<double, ACT_KIND_TANH>(plan, L, dims, W, b, X, Y, y_sm, gx, losses, B, iters, rate, head, s);
    else launch_induce_t<float, ACT_KIND_TANH>(plan, L, dims, W, b, X, Y, y_sm, gx, losses, B, iters, rate, head, s);
  } else {
    if (dtype == TO_F64) launch_induce_t<double, ACT_KIND_LOGISTIC>(plan, L, dims, W, b, X, Y, y_sm, gx, losses, B, iters, rate, head, s);
    else launch_induce_t<float, ACT_KIND_LOGISTIC>(plan, L, dims, W, b, X, Y, y_sm, gx, losses, B, iters, rate, head, s);
  }
  TO_HIP(hipGetLastError());
  count_launch();
}

// after the stream has been synchronised: 0, or the iteration (1-based) at which a workgroup gave up waiting (and its row)
int64_t induce_seq_status(int64_t* row) {
  if (!g_in.status || g_in.status[0] == 0) return 0;
  if (row) *row = g_in.status[1];
  return g_in.status[0];
}

}  // namespace to
