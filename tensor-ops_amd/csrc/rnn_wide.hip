// The recurrence of a WIDE `fullyConnected` layer (Recurrent.hs:91-119) over a whole sequence: rnn_seq.hip's contraction
//   out_t[r][j] = epilogue(sum_k v_{t-1}[r][k] M[k][j])      (M = W'^T forward, W' reverse; Z [T][B][H], St [T+1][B][H])
// for the widths at which W' no longer fits ONE workgroup's LDS (fp32 H >= 202, fp64 H >= 143), where rnn_seq_kernel streams
// W' from L2 every step and loses to the per-step route (profiles/r07_rnn_scan.txt).  Here W' is split by COLUMNS over the
// G <= 32 workgroups of a group, ONE launch per layer and direction whatever T:
//
//   * a GROUP of G workgroups (512 threads each) serves R <= 16 rows (sequences).  Workgroup g owns the column slab
//     J_g = [g C, g C + C) of C = ceil(H / G) columns: it loads M[:, J_g] into LDS once ([H][Cp], k-major: a wave of the FMA
//     form reads 64 consecutive j of one k, conflict-free for any Cp = C; the MFMA form pads the slab to whole 16-column
//     blocks with Cp = 16 (mod 32), so that the four k rows of an operand fall into the two halves of the banks) and keeps
//     it there for all T steps, beside two buffers [R][H | 1] for v_{t-1} / v_t and the cross-wave reduction scratch;
//   * up to 8 groups run side by side (B <= 8 R): group q is the workgroups with blockIdx & 7 == q of a grid of 8 G -- the
//     placement xcd_placement_ok() vouches for, every group behind one XCD's L2.  Workgroups of unused groups return
//     at once.  Placement is a performance precondition; correctness rests on agent-scope atomics only;
//   * the inner product has two forms, by R, each with a summation order fixed by the plan (dtype, H, B, min_groups), so a
//     result depends neither on the workgroups' timing nor on the other rows:
//       R <= 4, FMA form: thread (slice, column) walks its K slice with acc[R] in registers -- M from LDS with lanes along
//         j, v an LDS broadcast;
//       5 <= R <= 16, MFMA form: v_mfma_f32_16x16x4_f32 / v_mfma_f64_16x16x4_f64, rows padded to 16 in registers; a wave
//         takes one 16-column block and a K slice, both operands from LDS;
//     the K slices' partial sums then meet in LDS and are added in slice order by the thread that owns (row, column);
//   * the epilogue is rnn_seq_kernel's, store for store: the P_t / G_t element was loaded one step ahead, z / dz goes to Z in
//     place, act(z) to St (forward), acc act'(St) + G to Z (reverse); the new value goes into the workgroup's own next-state
//     buffer directly and, as tagged words, to the mates.
//
// The exchange is xcd_exchange.hpp's, into exch[parity of the step][group][row][column]: every workgroup gathers the other
// slabs' words into its next-state buffer, eight words a thread in flight.  The last step publishes nothing.  G = 1 never
// arises: those widths are rnn_seq_kernel's.  A wait that runs out stores {step + 1, the launch's id + 1} into a host-visible
// status pair (the first report of a call is kept) and the workgroup leaves its step loop; Z and St are then unspecified.
//
// Which (dtype, H) have a plan (rnn_wide_plan below): above rnn_seq_plan's LDS range, H <= RNN_SEQ_MAX_H, B <= 128, and some
// G <= 32 whose slab fits 160 KiB beside the rows' buffers.  fp32: every H in 202 .. 1024 for B <= 8 (R = 1); at H = 1024
// the G = 32 slab is 128 KiB and at most R = 3 rows fit beside it (B <= 24).  fp64: above H = 768 a G = 32 slab no longer
// fits 160 KiB beside one row's buffers (H = 1024: 256 KiB), so fp64 stops at H = 768 -- wider layers keep the per-step route.
#include <algorithm>
#include <cstdlib>
#include <type_traits>

#include "common.hpp"
#include "devmath.hpp"
#include "xcd_exchange.hpp"

namespace to {

namespace {

constexpr int RW_THREADS = 512, RW_NW = RW_THREADS / 64;
constexpr int RW_QMAX = 4;         // (row, column) items of its slab a thread finishes: R * C <= RW_QMAX * RW_THREADS
constexpr int RW_FLIGHT = 8;       // exchange words a thread keeps in flight
constexpr int RW_MAX_SLICES = 16;  // K slices of the FMA form
constexpr int64_t RW_LDS_MAX = 160 * 1024;

typedef float rw_f32x4 __attribute__((ext_vector_type(4)));
typedef double rw_f64x4 __attribute__((ext_vector_type(4)));

template <class S>
struct RnnWideArgs {
  const S* M;  // [H][H]: out[j] = sum_k v[k] M[k][j]
  S* Z;        // [T][B][H]: forward P -> z, reverse G -> dz, in place
  S* St;       // [T+1][B][H]: forward writes blocks 1..T from block 0; reverse reads blocks 1..T
  long B, T;
  int H, G, C, Cp, R, groups, nsl, klen;
  unsigned long long* exch;  // [2][groups][R][H][words of S]: {tag, 32 bits of the value}, zero at launch
  long long* status;         // host-visible: [0] nonzero = a wait ran out at that step + 1, [1] the launch's id + 1
  long long timeout;         // wall_clock64 ticks
  long long id;
};

// this thread's K slice of its column for RR rows: M from LDS (lanes along j), v an LDS broadcast
template <class S, int RR>
__device__ __forceinline__ void rw_fma_slice(const S* __restrict__ Ms, const S* __restrict__ vc, S* __restrict__ red, int Cp,
                                             int Hs, int jl, int sl, int k0, int k1) {
  S acc[RR];
#pragma unroll
  for (int r = 0; r < RR; ++r) acc[r] = S(0);
#pragma unroll 4
  for (int k = k0; k < k1; ++k) {
    const S m = Ms[(long)k * Cp + jl];
#pragma unroll
    for (int r = 0; r < RR; ++r) acc[r] = dm::fma(vc[r * Hs + k], m, acc[r]);
  }
#pragma unroll
  for (int r = 0; r < RR; ++r) red[((long)sl * RR + r) * Cp + jl] = acc[r];
}

__device__ __forceinline__ rw_f32x4 rw_mfma(float a, float b, rw_f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
__device__ __forceinline__ rw_f64x4 rw_mfma(double a, double b, rw_f64x4 c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }

template <class S, bool REV, bool MFMA, int ACT>
__global__ __launch_bounds__(RW_THREADS) void rnn_wide_kernel(RnnWideArgs<S> a) {
  const int q = blockIdx.x & 7, g = blockIdx.x >> 3;
  if (q >= a.groups) return;
  extern __shared__ __align__(16) unsigned char rw_lds[];
  constexpr int WORDS = sizeof(S) / 4;
  using V4 = typename std::conditional<sizeof(S) == 8, rw_f64x4, rw_f32x4>::type;
  const int H = a.H, R = a.R, C = a.C, Cp = a.Cp, Hs = H | 1, nsl = a.nsl;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j0 = g * C, nc = min(C, H - j0);   // (the plan leaves no workgroup without columns: nc >= 1)
  const long b0 = (long)q * R;
  const int rows = (int)min((long)R, a.B - b0);
  const long blk = a.B * (long)H;              // one time step of Z / St
  // ---- LDS layout (rnn_wide_plan counts the same items) ------------------------------------------------------------------
  S* Ms = reinterpret_cast<S*>(rw_lds);        // [H][Cp]: M[:, J_g], zero behind column nc
  S* v = Ms + (long)H * Cp;                    // [2][R][Hs]
  S* red = v + 2 * (long)R * Hs;               // [nsl][R][Cp]
  S* flag = red + (long)nsl * R * Cp;          // a wait ran out (only ever set)
  for (int e = tid; e < H * Cp; e += RW_THREADS) {
    const int k = e / Cp, c = e - k * Cp;
    Ms[e] = c < nc ? a.M[(long)k * H + j0 + c] : S(0);
  }
  // v_{-1}: the initial states (forward) or dz_T = 0 (reverse); rows this group does not have stay zero in both buffers
  for (int e = tid; e < 2 * R * Hs; e += RW_THREADS) {
    const int r = e / Hs, k = e - r * Hs;
    v[e] = (!REV && r < rows && k < H) ? a.St[(b0 + r) * H + k] : S(0);
  }
  if (tid == 0) *flag = S(0);
  // the (row, column) items this thread finishes, and their first addend
  int rq[RW_QMAX], jq[RW_QMAX];
  bool live[RW_QMAX];
  S pre[RW_QMAX];
#pragma unroll
  for (int u = 0; u < RW_QMAX; ++u) {
    const int item = tid + u * RW_THREADS;
    rq[u] = item / C;
    jq[u] = item - rq[u] * C;
    live[u] = rq[u] < rows && jq[u] < nc;
    const long t0 = REV ? a.T - 1 : 0;
    pre[u] = live[u] ? a.Z[t0 * blk + (b0 + rq[u]) * H + j0 + jq[u]] : S(0);
  }
  __syncthreads();
  const int others = H - nc, total = rows * others;   // what the mates own of a step's [rows][H]
  int cur = 0;
  for (long step = 0; step < a.T; ++step) {
    const long t = REV ? a.T - 1 - step : step;
    const S* vc = v + (long)cur * R * Hs;
    S* vn = v + (long)(cur ^ 1) * R * Hs;
    const bool product = !REV || step > 0;   // (dz_T = 0: the reverse's first step has no product, as in rnn_seq_kernel)
    // ---- the K slices' partial products into red -----------------------------------------------------------------------
    if (product) {
      if constexpr (!MFMA) {
        if (tid < nsl * C) {
          const int sl = tid / C, jl = tid - sl * C, k0 = sl * a.klen, k1 = min(H, k0 + a.klen);
          switch (R) {
            case 1: rw_fma_slice<S, 1>(Ms, vc, red, Cp, Hs, jl, sl, k0, k1); break;
            case 2: rw_fma_slice<S, 2>(Ms, vc, red, Cp, Hs, jl, sl, k0, k1); break;
            case 3: rw_fma_slice<S, 3>(Ms, vc, red, Cp, Hs, jl, sl, k0, k1); break;
            default: rw_fma_slice<S, 4>(Ms, vc, red, Cp, Hs, jl, sl, k0, k1); break;
          }
        }
      } else {
        // A lane l = v[i = l & 15][k + (l >> 4)], B lane l = M[k + (l >> 4)][16 jb + (l & 15)]; D register r of lane l is row
        // 4 (l >> 4) + r (fp32) or (l >> 4) + 4 r (fp64), column l & 15
        const int nb = (C + 15) / 16, i = lane & 15, kg = lane >> 4;
        for (int it = wave; it < nb * nsl; it += RW_NW) {
          const int sl = it / nb, jb = it - sl * nb, k0 = sl * a.klen, k1 = min(H, k0 + a.klen);
          V4 acc = {S(0), S(0), S(0), S(0)};
          for (int k = k0; k < k1; k += 4) {
            const int kk = k + kg;
            const bool in = kk < k1;
            const S av = (in && i < R) ? vc[i * Hs + kk] : S(0);
            const S bv = in ? Ms[(long)kk * Cp + jb * 16 + i] : S(0);
            acc = rw_mfma(av, bv, acc);
          }
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int row = sizeof(S) == 8 ? kg + 4 * r : 4 * kg + r;
            if (row < R) red[((long)sl * R + row) * Cp + jb * 16 + i] = acc[r];
          }
        }
      }
    }
    __syncthreads();
    // ---- the slices in order, the epilogue, the publication -------------------------------------------------------------
    const bool more = step + 1 < a.T;
    const unsigned tag = (unsigned)(step + 1);
    unsigned long long* ex = a.exch + (((step & 1) * (long)a.groups + q) * R) * H * WORDS;   // this group's [R][H][WORDS]
#pragma unroll
    for (int u = 0; u < RW_QMAX; ++u) {
      if (live[u]) {
        const int r = rq[u], jl = jq[u], j = j0 + jl;
        const long off = t * blk + (b0 + r) * H + j;
        S acc = S(0);
        if (product)
          for (int sl = 0; sl < nsl; ++sl) acc += red[((long)sl * R + r) * Cp + jl];
        S o;
        if (!REV) {
          const S z = pre[u] + acc;
          a.Z[off] = z;
          if constexpr (ACT == ACT_KIND_TANH) o = dm::tanh_act(z);
          else o = dm::logistic(z);
          a.St[off + blk] = o;
        } else {
          const S h = a.St[off + blk];
          if constexpr (ACT == ACT_KIND_TANH) o = dm::fma(acc, dm::tanh_dact(h), pre[u]);
          else o = dm::fma(acc * h, S(1) - h, pre[u]);
          a.Z[off] = o;
        }
        if (more) {
          vn[r * Hs + j] = o;
          unsigned wd[WORDS];   // (xe::publish written out: as a call, in each form tried, this file's address arithmetic moves)
          __builtin_memcpy(wd, &o, sizeof(S));
#pragma unroll
          for (int w = 0; w < WORDS; ++w)
            __hip_atomic_store(ex + ((long)r * H + j) * WORDS + w, ((unsigned long long)tag << 32) | wd[w], __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
        }
      }
    }
    // ---- the mates' slabs of v_t into the next-state buffer ------------------------------------------------------------
    // (the poll is written out: on a shared primitive, in each shape tried, this file's assembly moves -- xcd_exchange.hpp)
    bool ok = true;
    if (more) {
      constexpr int NV = RW_FLIGHT / WORDS;   // values in flight
      const long long c0 = wall_clock64();
      for (int base = tid; base < total && ok; base += RW_THREADS * NV) {
        long src[NV];
        int dst[NV];
        unsigned long long wv[NV][WORDS];
        bool have[NV][WORDS];
#pragma unroll
        for (int n = 0; n < NV; ++n) {
          const int e = base + n * RW_THREADS;
          const bool in = e < total;
          const int r = in ? e / others : 0, x = in ? e - r * others : 0, j = x < j0 ? x : x + nc;
          src[n] = ((long)r * H + j) * WORDS;
          dst[n] = in ? r * Hs + j : -1;
#pragma unroll
          for (int w = 0; w < WORDS; ++w) { wv[n][w] = 0ull; have[n][w] = !in; }
        }
        while (true) {
#pragma unroll
          for (int n = 0; n < NV; ++n)
#pragma unroll
            for (int w = 0; w < WORDS; ++w)
              if (!have[n][w]) wv[n][w] = __hip_atomic_load(ex + src[n] + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          bool all = true;
#pragma unroll
          for (int n = 0; n < NV; ++n)
#pragma unroll
            for (int w = 0; w < WORDS; ++w) {
              if (!have[n][w]) have[n][w] = (unsigned)(wv[n][w] >> 32) == tag;
              all = all && have[n][w];
            }
          if (all) break;
          if (wall_clock64() - c0 > a.timeout) {
            ok = false;
            break;
          }
          __builtin_amdgcn_s_sleep(1);
        }
        if (ok) {
#pragma unroll
          for (int n = 0; n < NV; ++n)
            if (dst[n] >= 0) {
              unsigned wd[WORDS];
#pragma unroll
              for (int w = 0; w < WORDS; ++w) wd[w] = (unsigned)wv[n][w];
              S x;
              __builtin_memcpy(&x, wd, sizeof(S));
              vn[dst[n]] = x;
            }
        }
      }
      if (!ok) *flag = S(1);
      // the next step's addend, requested behind the step's last wait on memory and back before the next epilogue
      const long tn = REV ? t - 1 : t + 1;
#pragma unroll
      for (int u = 0; u < RW_QMAX; ++u)
        if (live[u]) pre[u] = a.Z[tn * blk + (b0 + rq[u]) * H + j0 + jq[u]];
    }
    __syncthreads();
    if (*flag != S(0)) {   // a mate never showed up (uniform: read behind the barrier); the first report of a call is kept
      if (tid == 0 && a.status[0] == 0) {
        a.status[1] = a.id + 1;
        a.status[0] = step + 1;
      }
      return;
    }
    cur ^= 1;
  }
}

xe::XcdExchange g_rw(false);

template <class S, bool REV, bool MFMA, int ACT>
void rw_go(const RnnWidePlan& p, const void* M, void* Z, void* St, int64_t B, int64_t T, int64_t H, int64_t id, hipStream_t s) {
  xe::allow_full_lds<rnn_wide_kernel<S, REV, MFMA, ACT>>();
  RnnWideArgs<S> a{(const S*)M, (S*)Z, (S*)St, (long)B, (long)T, (int)H, p.G, p.C, p.Cp, p.R, p.groups, p.nsl, p.klen,
                   g_rw.exch(), g_rw.status_dev<long long>(), xe::watchdog_ticks(), (long long)id};
  launch_k(rnn_wide_kernel<S, REV, MFMA, ACT>, dim3((unsigned)(8 * p.G)), dim3(RW_THREADS), p.lds_bytes, s, a);
}

template <class S, bool REV, bool MFMA>
void rw_go_act(int act_kind, const RnnWidePlan& p, const void* M, void* Z, void* St, int64_t B, int64_t T, int64_t H, int64_t id,
               hipStream_t s) {
  if (act_kind == ACT_KIND_TANH) rw_go<S, REV, MFMA, ACT_KIND_TANH>(p, M, Z, St, B, T, H, id, s);
  else rw_go<S, REV, MFMA, ACT_KIND_LOGISTIC>(p, M, Z, St, B, T, H, id, s);
}

template <class S>
void rw_go_type(bool reverse, int act_kind, const RnnWidePlan& p, const void* M, void* Z, void* St, int64_t B, int64_t T,
                int64_t H, int64_t id, hipStream_t s) {
  if (reverse) p.mfma ? rw_go_act<S, true, true>(act_kind, p, M, Z, St, B, T, H, id, s) : rw_go_act<S, true, false>(act_kind, p, M, Z, St, B, T, H, id, s);
  else p.mfma ? rw_go_act<S, false, true>(act_kind, p, M, Z, St, B, T, H, id, s) : rw_go_act<S, false, false>(act_kind, p, M, Z, St, B, T, H, id, s);
}

}  // namespace

// R = ceil(B / min(8, B)) rows a group (the rows spread over the 8 XCDs before a group takes a second one), FMA form up to
// R = 4.  G: the smallest of 2, 4, 8, 16, 32 -- raised to at least min_groups -- at which the slab, the R rows' two buffers
// and the reduction scratch fit 160 KiB; then lowered until no workgroup is without columns (G = ceil(H / C)).
bool rnn_wide_plan(int dtype, int64_t H, int64_t B, int min_groups, RnnWidePlan* p) {
  *p = RnnWidePlan();
  if (H < 1 || H > RNN_SEQ_MAX_H || B < 1 || B > 8 * 16 || min_groups < 0 || min_groups > 32) return false;
  RnnSeqPlan seq;
  if (rnn_seq_plan(dtype, H, B, &seq) && seq.m_lds) return false;   // rnn_seq_kernel holds W' in one workgroup's LDS
  const int64_t es = dtype == TO_F64 ? 8 : 4;
  const int64_t R = (B + std::min<int64_t>(8, B) - 1) / std::min<int64_t>(8, B);
  const bool mfma = R > 4;
  for (int64_t G0 = 2; G0 <= 32; G0 *= 2) {
    const int64_t Gt = std::min<int64_t>(std::max<int64_t>(G0, min_groups), H);
    const int64_t C = (H + Gt - 1) / Gt, G = (H + C - 1) / C;
    if (G < 2 || C > RW_THREADS || R * C > RW_QMAX * RW_THREADS) continue;
    int64_t Cp = C, nsl, klen;
    if (mfma) {
      const int64_t nb = (C + 15) / 16;
      Cp = 16 * nb + (nb % 2 == 0 ? 16 : 0);
      nsl = nb >= RW_NW ? 1 : RW_NW / nb;
      klen = ((H + nsl - 1) / nsl + 3) / 4 * 4;
    } else {
      nsl = std::min<int64_t>(RW_THREADS / C, RW_MAX_SLICES);
      klen = (H + nsl - 1) / nsl;
    }
    const int64_t elems = H * Cp + 2 * R * (H | 1) + nsl * R * Cp + 2;
    if (elems * es > RW_LDS_MAX) continue;
    p->exists = true;
    p->G = (int)G; p->C = (int)C; p->Cp = (int)Cp; p->R = (int)R;
    p->groups = (int)((B + R - 1) / R);
    p->nsl = (int)nsl; p->klen = (int)klen;
    p->mfma = mfma;
    p->lds_bytes = (size_t)(elems * es);
    return true;
  }
  return false;
}

// the status pair back to "no report": the driver calls it before a call's first launch (nothing is in flight then)
void rnn_wide_begin() { g_rw.status_reset(); }

// after the stream has been synchronised: 0, or the step (1-based) at which a workgroup gave up waiting, and that launch's id
int64_t rnn_wide_status(int64_t* id) {
  const long long* st = g_rw.status<long long>();
  if (!st || st[0] == 0) return 0;
  if (id) *id = st[1] - 1;
  return st[0];
}

void launch_rnn_wide(int dtype, bool reverse, const RnnWidePlan& p, const void* M, void* Z, void* St, int64_t B, int64_t T,
                     int64_t H, int act_kind, int64_t id, hipStream_t s) {
  if (B == 0 || T == 0) return;
  TO_CHECK(act_kind == ACT_KIND_LOGISTIC || act_kind == ACT_KIND_TANH, TO_ERR_ARG, "rnn_wide: unknown state activation");
  TO_CHECK(p.exists && p.G >= 2 && p.G <= 32 && p.R >= 1 && p.R <= 16 && p.groups >= 1 && p.groups <= 8 &&
               (int64_t)p.groups * p.R >= B && (int64_t)p.G * p.C >= H && (int64_t)(p.G - 1) * p.C < H && p.Cp >= p.C &&
               p.lds_bytes <= (size_t)RW_LDS_MAX && T < 4000000000LL,
           TO_ERR_STATE, "rnn_wide: not a plan of rnn_wide_plan for this shape");
  const size_t need = (size_t)2 * p.groups * p.R * H * (dtype == TO_F64 ? 2 : 1) * 8;
  g_rw.reserve(need);
  // (a kernel launch, not XcdExchange::zero(): the launch count and the call trace of the wide route name it)
  launch_fill(TO_F32, g_rw.exch(), (int64_t)(need / 4), 0.0, s);
  if (dtype == TO_F64) rw_go_type<double>(reverse, act_kind, p, M, Z, St, B, T, H, id, s);
  else rw_go_type<float>(reverse, act_kind, p, M, Z, St, B, T, H, id, s);
  TO_HIP(hipGetLastError());
  count_launch();
}

}  // namespace to
