// Per-sequence training of a recurrent stack (to_rnn_stack_online_sgd, route B): `foldl' trainNetwork'` over n_idx sequences
// -- forward over T steps, BPTT, the update -- as ONE launch by ONE workgroup.  The loop is a dependent chain of single
// sequences, so there is nothing to spread over workgroups and nothing crosses one: no spin, no flag, no residency
// requirement; the kernel waits on nothing but its own barriers.
//   rnn_online_kernel : LDS holds, for the whole call, every layer's W, W' and b and the stateful layers' learned initial
//                       states s (loaded once, written back once).  The matrices are k-major like rnn_gen_kernel's, M[k][j],
//                       with the leading dimension padded to an odd n | 1: the forward's consecutive threads read
//                       consecutive columns j, and the backward products W^T dz and W'^T dz -- one k a thread, walking j --
//                       read addresses an odd stride apart, never one bank.
//   What is computed  : per step t and layer, z = W a + W' s + b in rnn_gen_kernel's fixed order -- the input part by
//                       ascending k, the state part by ascending k, the bias --, new state state_act(z), output
//                       hidden_act(z); the head is loss_grad_rows_kernel's formulas.  A gradient element is the sum over
//                       ascending t of dz_t[j] in_t[k] (S_t[k] for W', 1 for b): no gradient buffer anywhere.  Every order
//                       is fixed, so the result is deterministic and does not depend on how a chain of sequences is cut
//                       into calls.
//   How it is looped  : only a stateful layer's own recurrence depends on the step before, so the kernel goes layer by
//                       layer, as the per-sequence route does, and keeps everything else off the chain.  Forward, layer l:
//                       the input parts of all T steps are (t, column) items spread over all threads (the sum stops after
//                       the input part and is parked on the tape); then, for a stateful layer, the recurrence serial in t
//                       -- a thread a column picks its parked sum up, adds the state part and the bias: the same chain of
//                       FMAs, bit for bit -- with ONE barrier a step, an LDS-only one (the step's hand-over is the state row
//                       in LDS; what goes to the tape is read behind the full barrier after the loop), and the next
//                       step's tape reads issued before this step's chain; then hidden_act of all steps as items again.
//                       The head: a wave a step, all steps at once.  Backward, layer L-1 down to 0: the recurrence
//                       dz_t += (W'^T dz_{t+1}) (.) state_act'(S_{t+1}) serial in t in the same way, s -= rate_state
//                       W'^T dz_0 at once (nothing reads s again before the next sequence), then the cotangent of the
//                       layer below for all (t, k) items.  Update, behind ONE barrier after the last read of the old
//                       parameters: a thread owns tiles of 4 x 4 elements (update_tiles).
//   The tape          : per step one record -- every layer's input row, every stateful layer's S_t (S_0 = s) and every
//                       layer's z_t, later dz_t, in one slot.  It lives in LDS where it fits beside the parameters, else in
//                       a pool buffer in global memory that only this workgroup touches (written, then read back behind a
//                       barrier).  Both homes sit behind one pointer; the template parameter TAPE_LDS only tells the
//                       compiler its address space (LDS or global instructions instead of flat ones, whose waits are
//                       all-or-nothing): the arithmetic is the same code and the kernel's range does not depend on T.  The
//                       vectors on the dependent chain -- the current state, the current dz -- are in LDS always.
//   Ragged            : to_rnn_stack_online_sgd_ragged's sequences have their own lengths.  The template parameter RAGGED
//                       gives every step loop above the sequence's own bound (a device table of n_idx lengths) and leaves
//                       T as the row stride; RAGGED = false is the dense entry's kernel as it was.  The plan is made for
//                       the longest length a call uses.
// ONLINE_THREADS = 512: the recurrences use a thread a column (at most ~200 columns fit the LDS) and pay for every wave at
// each barrier; the item phases and the update are throughput-bound (n m T FMAs a layer, two reads each) and want more
// than a wave a SIMD to hide the read latency.  512 is two waves a SIMD; 256 and 1024 have not been measured against it.
// Plain VALU FMAs from LDS (no MFMA form).
#include <algorithm>
#include <type_traits>

#include "common.hpp"
#include "devmath.hpp"

namespace to {

namespace {

constexpr int ONLINE_THREADS = 512;

// The (t, c) items of a [T][w] index space spread over the workgroup: thread tid takes items tid, tid + TH, ... with item
// i = (i / w, i % w), stepped without a division a turn.
template <int TH, class F>
__device__ __forceinline__ void for_items(long T, int w, int tid, F&& f) {
  long t = tid / w;
  int c = tid - (int)t * w;
  const int dt = TH / w, dc = TH - dt * w;
  while (t < T) {
    f(t, c);
    t += dt;
    c += dc;
    if (c >= w) { c -= w; ++t; }
  }
}
// A barrier whose hand-over is in LDS only: the workgroup's LDS accesses are done, its global stores need not be (they are
// read behind a later __syncthreads()).  A recurrence's per-step barrier.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// The update of one k-major matrix M[k][j] (W: k over the layer's inputs, src the input rows; W': k over the states, src
// S_t): M[k][j] -= rate * sum over ascending t of dz_t[j] src_t[k].  A thread owns tiles of 4 columns x 4 k: per step two
// 16-byte reads (the tape's rows start on 16-byte boundaries and are padded to four elements; what a ragged tile reads of
// the padding goes into sums that are never stored) feed 16 independent chains, each in its fixed order.
template <int TH, class S>
__device__ __forceinline__ void update_tiles(const S* tape, long rec, long T, int odz, int osrc, int n, int m, int ld, S* M,
                                             S rate, int tid) {
  const int nj = (n + 3) >> 2, nk = (m + 3) >> 2;
  for (int e = tid; e < nj * nk; e += TH) {
    const int kt = e / nj, j0 = 4 * (e - kt * nj), k0 = 4 * kt;
    S g[4][4] = {};
    const S* pd = tape + odz + j0;
    const S* px = tape + osrc + k0;
    for (long t = 0; t < T; ++t, pd += rec, px += rec) {
      const S* d = static_cast<const S*>(__builtin_assume_aligned(pd, 16));
      const S* x = static_cast<const S*>(__builtin_assume_aligned(px, 16));
      const S d0 = d[0], d1 = d[1], d2 = d[2], d3 = d[3];
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        const S xv = x[kk];
        g[kk][0] = dm::fma(d0, xv, g[kk][0]);
        g[kk][1] = dm::fma(d1, xv, g[kk][1]);
        g[kk][2] = dm::fma(d2, xv, g[kk][2]);
        g[kk][3] = dm::fma(d3, xv, g[kk][3]);
      }
    }
#pragma unroll
    for (int kk = 0; kk < 4; ++kk)
#pragma unroll
      for (int jj = 0; jj < 4; ++jj)
        if (k0 + kk < m && j0 + jj < n) M[(k0 + kk) * ld + j0 + jj] -= rate * g[kk][jj];
  }
}

template <class S>
struct RnnOnlineArgs {
  S* W[RNN_GEN_MAX_LAYERS];    // [n_l][n_{l-1}]
  S* WS[RNN_GEN_MAX_LAYERS];   // [n_l][n_l] (stateful)
  S* b[RNN_GEN_MAX_LAYERS];
  S* s[RNN_GEN_MAX_LAYERS];    // [n_l] (stateful): the learned initial state
  int n[RNN_GEN_MAX_LAYERS + 1];
  int sk[RNN_GEN_MAX_LAYERS];  // state activation, -1: stateless
  // LDS offsets (elements): W k-major [m][n | 1], W' k-major [n][n | 1], b, s, the state's two rows
  int w_off[RNN_GEN_MAX_LAYERS], ws_off[RNN_GEN_MAX_LAYERS], b_off[RNN_GEN_MAX_LAYERS], s_off[RNN_GEN_MAX_LAYERS],
      sc_off[RNN_GEN_MAX_LAYERS];
  // offsets within one step's tape record: the layer's input row, its state S_t, its z_t / dz_t
  int t_in[RNN_GEN_MAX_LAYERS], t_s[RNN_GEN_MAX_LAYERS], t_dz[RNN_GEN_MAX_LAYERS];
  const S* X;             // [N][T][n_0]
  const S* Y;             // [N][T][n_L]
  S* losses;              // [n_idx][T] or null
  const long long* idx;   // [n_idx] or null: sequences 0 .. n_idx-1
  S* tape;                // [T][rec] in global memory, or null: in LDS at tape_off
  long n_idx, T, rec;
  int L, vec_off, tape_off, hidden_kind, softmax;
  S rate_state, rate_params;
  const long long* lens;  // RAGGED: [n_idx], the steps of sequence idx[j]; the dense kernels never look at it
};

// RAGGED (to_rnn_stack_online_sgd_ragged): step js trains on the leading len = lens[js] steps of its sequence.  T stays what
// it is for the dense kernels in one place only -- the row stride of X, Y and losses --; every loop over steps runs to len,
// so the tape's records from len on, which an earlier, longer sequence left behind, are read by nothing; the head stores
// +0.0 into losses[js][len .. T).  len is the same value in every thread, so every barrier is still reached by all of them.
template <class S, bool TAPE_LDS, bool RAGGED>
__global__ __launch_bounds__(ONLINE_THREADS) void rnn_online_kernel(RnnOnlineArgs<S> a) {
  extern __shared__ __align__(16) unsigned char online_lds[];
  S* const lds = reinterpret_cast<S*>(online_lds);
  constexpr int TH = ONLINE_THREADS;
  const int L = a.L, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, hk = a.hidden_kind;
  const int n0 = a.n[0], nL = a.n[L];
  const long T = a.T, rec = a.rec;   // T: the rows of a sequence in X, Y and losses
  // ---- the parameters and the initial states, once --------------------------------------------------------------------
  for (int l = 0; l < L; ++l) {
    const int m = a.n[l], n = a.n[l + 1], ld = n | 1;
    S* Wk = lds + a.w_off[l];
    const S* W = a.W[l];
    for (int e = tid; e < n * m; e += TH) {
      const int j = e / m, k = e - j * m;
      Wk[k * ld + j] = W[e];
    }
    if (a.sk[l] >= 0) {
      S* WSk = lds + a.ws_off[l];
      const S* WS = a.WS[l];
      for (int e = tid; e < n * n; e += TH) {
        const int j = e / n, k = e - j * n;
        WSk[k * ld + j] = WS[e];
      }
      for (int e = tid; e < n; e += TH) lds[a.s_off[l] + e] = a.s[l][e];
    }
    for (int e = tid; e < n; e += TH) lds[a.b_off[l] + e] = a.b[l][e];
  }
  // The tape: element (t, o) at t * rec + o.  The one accessor of both homes.
  S* const tape = TAPE_LDS ? lds + a.tape_off : a.tape;
  __syncthreads();

  for (long js = 0; js < a.n_idx; ++js) {
    const long q = a.idx ? (long)a.idx[js] : js;
    const S* Xq = a.X + q * T * n0;
    const S* Yq = a.Y + q * T * nL;
    long len = T;   // the sequence's steps
    if constexpr (RAGGED) len = (long)a.lens[js];
    // ---- the sequence's rows of X onto the tape; S_0 = s: the current state and the tape's first record -------------------
    {
      const int o0 = a.t_in[0];
      for_items<TH>(len, n0, tid, [&](long t, int e) { tape[t * rec + o0 + e] = Xq[t * n0 + e]; });
    }
    for (int l = 0; l < L; ++l) {
      if (a.sk[l] < 0) continue;
      const int n = a.n[l + 1];
      for (int e = tid; e < n; e += TH) {
        const S v = lds[a.s_off[l] + e];
        lds[a.sc_off[l] + e] = v;
        tape[a.t_s[l] + e] = v;
      }
    }
    __syncthreads();
    // ---- forward, layer by layer -----------------------------------------------------------------------------------------
    for (int l = 0; l < L; ++l) {
      const int m = a.n[l], n = a.n[l + 1], ld = n | 1, sk = a.sk[l];
      const bool last = l + 1 == L;
      const S* Wk = lds + a.w_off[l];
      const S* bb = lds + a.b_off[l];
      const int oin = a.t_in[l], odz = a.t_dz[l], onx = last ? 0 : a.t_in[l + 1];
      // the input parts of all steps (a stateless layer: all of z, and what comes behind it)
      for_items<TH>(len, n, tid, [&](long t, int j) {
        S* const rt = tape + t * rec;
        const S* in = static_cast<const S*>(__builtin_assume_aligned(rt + oin, 16));
        const S* wj = Wk + j;
        S acc = S(0);
#pragma unroll 8
        for (int k = 0; k < m; ++k) acc = dm::fma(in[k], wj[k * ld], acc);
        if (sk >= 0) {
          rt[odz + j] = acc;   // parked: the recurrence goes on from here
        } else {
          const S z = acc + bb[j];
          if (last) rt[odz + j] = z;
          else rt[onx + j] = dm::act(hk, z);
        }
      });
      __syncthreads();
      if (sk < 0) continue;
      // the recurrence: z_t = (parked sum) + W' S_t + b, S_{t+1} = state_act(z_t); a thread a column (n <= TH: the plan)
      {
        const S* WSk = lds + a.ws_off[l];
        const int os = a.t_s[l], sq = (n + 3) & ~3;
        S* const sc0 = lds + a.sc_off[l];
        const bool mine = tid < n;
        const S* vj = WSk + tid;
        const S bj = mine ? bb[tid] : S(0);
        S pz = mine ? tape[odz + tid] : S(0);
        for (long t = 0; t < len; ++t) {
          S* const rt = tape + t * rec;
          const bool more = t + 1 < len;
          const int cs = (int)(t & 1);
          const S* sc = static_cast<const S*>(__builtin_assume_aligned(sc0 + cs * sq, 16));
          S* sn = sc0 + (cs ^ 1) * sq;
          S pnext = S(0);
          if (mine && more) pnext = rt[rec + odz + tid];   // the next step's parked sum, off its chain
          if (mine) {
            S acc = pz;
#pragma unroll 8
            for (int k = 0; k < n; ++k) acc = dm::fma(sc[k], vj[k * ld], acc);
            const S z = acc + bj;
            const S ns = dm::act(sk, z);
            sn[tid] = ns;
            if (more) rt[rec + os + tid] = ns;   // S_{t+1}
            rt[odz + tid] = z;
          }
          lds_barrier();
          pz = pnext;
        }
      }
      __syncthreads();
      if (!last) {   // hidden_act(z) of all steps: the next layer's input rows
        for_items<TH>(len, n, tid, [&](long t, int j) {
          S* const rt = tape + t * rec;
          rt[onx + j] = dm::act(hk, rt[odz + j]);
        });
        __syncthreads();
      }
    }
    // ---- the head, a wave a step, all steps at once: z_L,t on the tape becomes dz_L,t in place; losses[js][t] -------------
    // (loss_grad_rows_kernel's formulas; a lane reads and writes its own elements only)
    if constexpr (RAGGED)
      if (a.losses)
        for (long t = len + tid; t < T; t += TH) a.losses[js * T + t] = S(0);   // padding: +0.0
    for (long t = wave; t < len; t += TH / 64) {
      S* const zr = tape + t * rec + a.t_dz[L - 1];
      const S* yr = Yq + t * nL;
      S l = S(0);
      if (a.softmax) {
        S mx = S(-INFINITY);
        for (int j = lane; j < nL; j += 64) mx = zr[j] > mx ? zr[j] : mx;
        mx = dm::wave_max(mx);
        S se = S(0), sy = S(0);
        for (int j = lane; j < nL; j += 64) {
          se += dm::exp(zr[j] - mx);
          sy += yr[j];
        }
        se = dm::wave_sum(se);
        sy = dm::wave_sum(sy);
        const S inv = S(1) / se, lse = dm::log(se);
        for (int j = lane; j < nL; j += 64) {
          const S d = zr[j] - mx, p = dm::exp(d) * inv;
          zr[j] = p * sy - yr[j];
          l += dm::ce_term(yr[j], d, lse);
        }
      } else {
        for (int j = lane; j < nL; j += 64) {
          const S sg = dm::logistic(zr[j]);
          const S e = yr[j] - sg;
          zr[j] = S(-2) * e * sg * (S(1) - sg);
          l += e * e;
        }
      }
      if (a.losses) {
        l = dm::wave_sum(l);
        if (lane == 0) a.losses[js * T + t] = l;
      }
    }
    __syncthreads();
    // ---- backward -----------------------------------------------------------------------------------------------------
    for (int l = L - 1; l >= 0; --l) {
      const int m = a.n[l], n = a.n[l + 1], ld = n | 1, sk = a.sk[l];
      const S* Wk = lds + a.w_off[l];
      const int odz = a.t_dz[l];
      if (sk >= 0) {   // dz_t += (W'^T dz_{t+1}) (.) state_act'(S_{t+1}), serial in t; then s -= rate_state W'^T dz_0
        const S* WSk = lds + a.ws_off[l];
        const int os = a.t_s[l], wq = (n + 3) & ~3;
        S* const d0 = lds + a.vec_off;
        const bool mine = tid < n;
        const S* vk = WSk + tid * ld;
        if (mine) d0[tid] = tape[(len - 1) * rec + odz + tid];
        S g0 = S(0), s1 = S(0);
        if (mine && len > 1) { g0 = tape[(len - 2) * rec + odz + tid]; s1 = tape[(len - 1) * rec + os + tid]; }
        __syncthreads();
        int cur = 0;
        for (long t = len - 2; t >= 0; --t) {
          S* const rt = tape + t * rec;
          const S* dcur = static_cast<const S*>(__builtin_assume_aligned(d0 + cur * wq, 16));
          S* dnxt = d0 + (cur ^ 1) * wq;
          S g0n = S(0), s1n = S(0);
          if (mine && t > 0) { g0n = rt[odz + tid - rec]; s1n = rt[os + tid]; }   // step t - 1's reads, off its chain
          if (mine) {
            S acc = S(0);
#pragma unroll 8
            for (int j = 0; j < n; ++j) acc = dm::fma(vk[j], dcur[j], acc);
            const S d = g0 + acc * dm::dact(sk, s1);
            dnxt[tid] = d;
            rt[odz + tid] = d;
          }
          lds_barrier();
          g0 = g0n; s1 = s1n;
          cur ^= 1;
        }
        if (mine) {
          const S* dcur = d0 + cur * wq;
          S acc = S(0);
#pragma unroll 8
          for (int j = 0; j < n; ++j) acc = dm::fma(vk[j], dcur[j], acc);
          lds[a.s_off[l] + tid] -= a.rate_state * acc;
        }
        __syncthreads();
      }
      if (l > 0) {   // dz_{l-1,t}[k] = (W^T dz_t)[k] hidden_act'(a_{l-1,t}[k]): time-independent, every (t, k) an item
        const int oin = a.t_in[l], odn = a.t_dz[l - 1];
        for_items<TH>(len, m, tid, [&](long t, int k) {
          S* const rt = tape + t * rec;
          const S* wk = Wk + k * ld;
          const S* dz = static_cast<const S*>(__builtin_assume_aligned(rt + odz, 16));
          const S h = rt[oin + k];
          S acc = S(0);
#pragma unroll 8
          for (int j = 0; j < n; ++j) acc = dm::fma(wk[j], dz[j], acc);
          rt[odn + k] = acc * dm::dact(hk, h);
        });
        __syncthreads();
      }
    }
    // ---- update: every read of the old parameters is behind a barrier above ---------------------------------------------
    for (int l = 0; l < L; ++l) {
      const int m = a.n[l], n = a.n[l + 1], ld = n | 1;
      const int odz = a.t_dz[l];
      update_tiles<TH>(tape, rec, len, odz, a.t_in[l], n, m, ld, lds + a.w_off[l], a.rate_params, tid);
      if (a.sk[l] >= 0) update_tiles<TH>(tape, rec, len, odz, a.t_s[l], n, n, ld, lds + a.ws_off[l], a.rate_params, tid);
      for (int j = tid; j < n; j += TH) {
        const S* p = tape;
        S g = S(0);
#pragma unroll 4
        for (long t = 0; t < len; ++t, p += rec) g += p[odz + j];
        lds[a.b_off[l] + j] -= a.rate_params * g;
      }
    }
    __syncthreads();
  }
  // ---- the parameters and the initial states back, once ----------------------------------------------------------------
  for (int l = 0; l < L; ++l) {
    const int m = a.n[l], n = a.n[l + 1], ld = n | 1;
    const S* Wk = lds + a.w_off[l];
    S* W = a.W[l];
    for (int e = tid; e < n * m; e += TH) {
      const int j = e / m, k = e - j * m;
      W[e] = Wk[k * ld + j];
    }
    if (a.sk[l] >= 0) {
      const S* WSk = lds + a.ws_off[l];
      S* WS = a.WS[l];
      for (int e = tid; e < n * n; e += TH) {
        const int j = e / n, k = e - j * n;
        WS[e] = WSk[k * ld + j];
      }
      for (int e = tid; e < n; e += TH) a.s[l][e] = lds[a.s_off[l] + e];
    }
    for (int e = tid; e < n; e += TH) a.b[l][e] = lds[a.b_off[l] + e];
  }
}

template <class S, bool TAPE_LDS, bool RAGGED>
void go_online(const RnnOnlinePlan& p, const RnnOnlineOperands& o, hipStream_t s) {
  static bool attr = false;
  if (!attr) {
    TO_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(rnn_online_kernel<S, TAPE_LDS, RAGGED>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)GEN_LDS_MAX));
    attr = true;
  }
  RnnOnlineArgs<S> a{};
  for (int l = 0; l < o.L; ++l) {
    a.W[l] = (S*)o.W[l]; a.WS[l] = (S*)o.WS[l]; a.b[l] = (S*)o.b[l]; a.s[l] = (S*)o.s[l];
    a.sk[l] = o.state_kind[l];
    a.w_off[l] = p.w_off[l]; a.ws_off[l] = p.ws_off[l]; a.b_off[l] = p.b_off[l]; a.s_off[l] = p.s_off[l];
    a.sc_off[l] = p.sc_off[l];
    a.t_in[l] = p.t_in[l]; a.t_s[l] = p.t_s[l]; a.t_dz[l] = p.t_dz[l];
  }
  for (int l = 0; l <= o.L; ++l) a.n[l] = (int)o.widths[l];
  a.X = (const S*)o.X; a.Y = (const S*)o.Y; a.losses = (S*)o.losses; a.idx = o.idx; a.tape = (S*)o.tape;
  a.n_idx = (long)o.n_idx; a.T = (long)o.T; a.rec = (long)p.rec;
  a.L = o.L; a.vec_off = p.vec_off; a.tape_off = p.tape_off; a.hidden_kind = o.hidden_kind;
  a.softmax = o.softmax ? 1 : 0;
  a.rate_state = (S)o.rate_state; a.rate_params = (S)o.rate_params;
  a.lens = o.lens;
  launch_k(rnn_online_kernel<S, TAPE_LDS, RAGGED>, dim3(1), dim3(ONLINE_THREADS), p.lds, s, a);
}

}  // namespace

// The LDS of the one workgroup, in elements: per layer W [m][n | 1], W' [n][n | 1] and s [n] (stateful), b [n]; then the
// vectors of the dependent chains, rows of a multiple of four elements from a 16-byte boundary -- the recurrence's dz twice
// at the widest stateful layer's width, and every stateful layer's current state twice --; then the tape (T records; in a
// record every row starts on a 16-byte boundary and is padded to four elements) where it still fits.  The plan fails when the
// parameters and those vectors alone exceed the limit, or a stateful layer has more columns than the workgroup has threads
// (its W' alone would be past the limit long before): T never decides that.
bool rnn_online_plan(int dtype, int L, const int64_t* widths, const int* stateful, int64_t T, RnnOnlinePlan* p) {
  if (L < 1 || L > RNN_GEN_MAX_LAYERS || T < 1) return false;
  for (int l = 0; l <= L; ++l)
    if (widths[l] < 1 || widths[l] > 65536) return false;
  const int64_t es = dtype == TO_F64 ? 8 : 4, cap = (int64_t)GEN_LDS_MAX / es;
  int64_t off = 0, rec = 0, ws = 0;
  auto up4 = [](int64_t v) { return (v + 3) & ~int64_t(3); };
  for (int l = 0; l < L; ++l) {
    const int64_t m = widths[l], n = widths[l + 1], ld = n | 1;
    if (stateful[l] && n > ONLINE_THREADS) return false;
    p->w_off[l] = (int)off; off += m * ld;
    p->ws_off[l] = (int)std::min(off, cap);
    if (stateful[l]) off += n * ld;
    if (off > cap) return false;
    p->b_off[l] = (int)off; off += n;
    p->s_off[l] = (int)off;
    if (stateful[l]) off += n;
    p->t_in[l] = (int)rec; rec += up4(m);
    p->t_s[l] = (int)rec;
    if (stateful[l]) { rec += up4(n); ws = std::max(ws, n); }
    p->t_dz[l] = (int)rec; rec += up4(n);
  }
  p->nmax = *std::max_element(widths + 1, widths + L + 1);
  off = up4(off);
  p->wpad = (int)up4(ws);
  p->vec_off = (int)off; off += 2 * up4(ws);
  for (int l = 0; l < L; ++l) {
    p->sc_off[l] = (int)std::min(off, cap);
    if (stateful[l]) off += 2 * up4(widths[l + 1]);
  }
  if (off > cap) return false;
  p->tape_off = (int)off;
  if (rec % 64 == 0) rec += 4;   // (rows of different steps not all in one bank)
  p->rec = rec;
  p->tape_elems = T * rec;
  p->tape_lds = T <= (cap - off) / rec;
  p->lds = (size_t)((off + (p->tape_lds ? p->tape_elems : 0)) * es);
  return true;
}

void launch_rnn_online(int dtype, const RnnOnlinePlan& p, const RnnOnlineOperands& o, hipStream_t s) {
  TO_CHECK(o.L >= 1 && o.L <= RNN_GEN_MAX_LAYERS && o.n_idx >= 1 && o.T >= 1 && p.lds <= GEN_LDS_MAX &&
               (p.tape_lds || o.tape != nullptr), TO_ERR_STATE, "internal: rnn_online outside its plan");
  auto go = [&](auto ragged) {
    constexpr bool R = decltype(ragged)::value;
    if (dtype == TO_F64) p.tape_lds ? go_online<double, true, R>(p, o, s) : go_online<double, false, R>(p, o, s);
    else p.tape_lds ? go_online<float, true, R>(p, o, s) : go_online<float, false, R>(p, o, s);
  };
  if (o.lens) go(std::true_type{});
  else go(std::false_type{});
  TO_HIP(hipGetLastError());
  count_launch();
}

}  // namespace to
