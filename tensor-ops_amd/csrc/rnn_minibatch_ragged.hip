// Minibatch training of a recurrent stack on sequences of their own lengths (to_rnn_stack_minibatch_sgd_ragged, route B): every
// update of a call as ONE launch by ONE workgroup, eight waves, on rnn_minibatch.hip's 16 x 16 x 4 MFMA blocks, with its stack
// in LDS (k-major, leading dimension 17 mod 32), its tape record, its layer-major loops and its one LDS-only barrier a
// recurrence step (rnn_minibatch_dev.hpp, rnn_minibatch_plan).  Nothing crosses workgroups; there is no spin.  What is this
// kernel's own is where a row lives:
//   Sorting   : the host sorts a minibatch's members by length, descending, stably by position in idx; rank q sits in slot q.
//               The sequences still running at step t are therefore a prefix q < act(t), act never grows with t, and the
//               minibatch's last step is Tk = the length of slot 0.
//   Packing   : step t owns P(t) = act(t) rounded up to 16 rows from row off(t) = sum_{t' < t} P(t') on: whole MFMA row blocks,
//               R_k = off(Tk) rows an update instead of T Mp.  The tape is sized for the call's largest R_k.
//   Padding   : rows act(t) <= q < P(t) of a step's last block carry zero input and a dz forced to zero behind the head, so
//               they add exactly +0 to every gradient and to gs, as rnn_minibatch.hip's rows q >= sz do.  They are never read
//               from X / Y and never written to losses.  (Such a row goes on from the state its slot left, with zero input: a
//               value of the state activation, finite; its dz chain is zero from its first step down.)
//   Row phases: the input projections, hidden_act, the head, the cotangents between layers and the update's row reductions
//               (mb_update, R = R_k) run over exactly R_k rows; none but the head and the load of X asks which step a row is of.
//               Those two read it from a table, one entry a row block.
//   Forward   : step t deals (P(t) / 16) x (Hp / 16) output blocks.  Slot q's state before step t is slot q of step t - 1's
//               block in LDS, which exists because P(t) <= P(t - 1); S_{t+1} goes to the tape only for the rows q < P(t + 1).
//               The loop ends at Tk.
//   Backward  : step t's row blocks below P(t + 1) take the carry (dz_{t+1} W') (.) act'(S_{t+1}); the blocks from P(t + 1) up
//               -- every sequence in them ends at t -- start their chain at G_t with no carry and no product.  Both kinds write
//               their dz block to the LDS buffer step t - 1 reads, so no row of it is ever a leftover of a later step.
//   gs        : the P(0) rows of dz_0 in ascending order (every length is at least 1: all sz sequences are among them).
//   Tables    : int32, built by rnn_minibatch_ragged_schedule below, uploaded once: per slot position k M + q the sequence, its
//               position j in idx (the row of losses) and its length; per minibatch Tk and where its off[0 .. Tk] and its
//               row-block -> step table begin.
//   losses    : zeroed by the host up front; the kernel writes losses[j][t] for t < the length only.
//   Determinism: every sum's order is fixed by (dtype, widths, M, the minibatch's lengths).  With every length T and n_idx a
//               multiple of M the layout is rnn_minibatch.hip's row for row (P(t) = Mp), and so is every sum.
#include <algorithm>
#include <numeric>
#include <vector>

#include "rnn_minibatch_dev.hpp"

namespace to {

namespace {

template <class S>
__global__ __launch_bounds__(MB_THREADS) void rnn_minibatch_ragged_kernel(RnnMinibatchArgs<S> a, const int* __restrict__ tab) {
  extern __shared__ __align__(16) unsigned char minibatch_ragged_lds[];
  S* const lds = reinterpret_cast<S*>(minibatch_ragged_lds);
  using V4 = mb_v4<S>;
  constexpr int TH = MB_THREADS, NW = MB_NW;
  const int L = a.L, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 15, g = lane >> 4, hk = a.hidden_kind;
  const int n0 = a.n[0], nL = a.n[L], Mp = a.Mp, hs = a.hs, blk = Mp * hs;
  const long T = a.T, rec = a.rec;
  S* const tape = a.tape;
  S* const ch0 = lds + a.chain_off;
  const V4 zero4 = {S(0), S(0), S(0), S(0)};
  const int* const t_seq = tab;
  const int* const t_pos = tab + a.n_idx;
  const int* const t_len = tab + 2 * a.n_idx;
  const int* const t_mb = tab + 3 * a.n_idx;
  mb_stack_in(a, lds, tid);

  long k0 = 0;
  for (long kk0 = 0; k0 < a.n_idx; k0 += a.M, ++kk0) {
    const int sz = (int)min(a.M, a.n_idx - k0);   // the minibatch's sequences: slots q < sz
    const int Tk = t_mb[2 * kk0];
    const int* const off = tab + t_mb[2 * kk0 + 1];   // off[0 .. Tk]: a step's first row
    const int* const bt = off + Tk + 1;               // row block -> its step
    const long R = off[Tk];
    const int P0 = off[1];
    // slot q (< sz) runs at step t?  (a row of a step's last block beyond that is padding)
    auto runs = [&](int q, int t) { return q < sz && t < t_len[k0 + q]; };
    // ---- the rows of X onto the tape (padding rows: zeros); S_0 = s in every row of step 0 ---------------------------------
    {
      const int w0 = (n0 + 3) & ~3, o0 = a.t_in[0];
      for (long e = tid; e < R * w0; e += TH) {
        const long r = e / w0;
        const int j = (int)(e - r * w0), t = bt[r >> 4], q = (int)(r - off[t]);
        S v = S(0);
        if (j < n0 && runs(q, t)) v = a.X[((long)t_seq[k0 + q] * T + t) * n0 + j];
        tape[r * rec + o0 + j] = v;
      }
    }
    for (int l = 0; l < L; ++l) {
      if (a.sk[l] < 0) continue;
      const int n = a.n[l + 1], n4 = (n + 3) & ~3;
      for (int e = tid; e < P0 * n4; e += TH) {
        const int q = e / n4, j = e - q * n4;
        tape[q * rec + a.t_s[l] + j] = j < n ? lds[a.s_off[l] + j] : S(0);
      }
    }
    __syncthreads();
    // ---- forward, layer by layer -----------------------------------------------------------------------------------------
    for (int l = 0; l < L; ++l) {
      const int m = a.n[l], n = a.n[l + 1], ld = a.ld[l], sk = a.sk[l];
      const int m4 = (m + 3) & ~3, n4 = (n + 3) & ~3, ncb = (n + 15) >> 4;
      const bool last = l + 1 == L;
      const S* Wk = lds + a.w_off[l];
      const S* bb = lds + a.b_off[l];
      const int oin = a.t_in[l], odz = a.t_dz[l], onx = last ? 0 : a.t_in[l + 1];
      if (sk >= 0)   // the state block: s in every row, zeros behind column n; the other buffer zeros
        for (int e = tid; e < 2 * blk; e += TH) {
          const int j = e % hs;
          ch0[e] = (e < blk && j < n) ? lds[a.s_off[l] + j] : S(0);
        }
      // the input parts of all R rows (a stateless layer: all of z, and what comes behind it)
      {
        const long ntile = (R >> 4) * ncb;
        for (long it = wave; it < ntile; it += NW) {
          const long rb = it / ncb;
          const int cb = (int)(it - rb * ncb), j = cb * 16 + c;
          const S* arow = tape + (rb * 16 + c) * rec + oin;
          const S* bcol = Wk + j;
          V4 acc = zero4;
#pragma unroll 4
          for (int k = g; k < m4; k += 4) acc = mb_mfma(arow[k], bcol[k * ld], acc);
          if (j < n4) {
            const S bj = j < n ? bb[j] : S(0);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              S* const rt = tape + (rb * 16 + mb_row<S>(g, r)) * rec;
              if (sk >= 0) {
                rt[odz + j] = acc[r];   // parked: the recurrence goes on from here
              } else {
                const S z = acc[r] + bj;
                if (last) rt[odz + j] = j < n ? z : S(0);
                else rt[onx + j] = j < n ? dm::act(hk, z) : S(0);
              }
            }
          }
        }
      }
      __syncthreads();
      if (sk < 0) continue;
      // the recurrence: z_t = (parked block) + S_t W'^T + b, S_{t+1} = state_act(z_t), on step t's P(t) rows
      {
        const S* WSk = lds + a.ws_off[l];
        const int os = a.t_s[l];
        auto parked = [&](int row0, int it) {   // row0: the step's first row
          const int qb = it / ncb, j = (it - qb * ncb) * 16 + c;
          V4 v = zero4;
          if (j < n4) {
            const S* p = tape + (long)(row0 + qb * 16) * rec + odz + j;
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = p[mb_row<S>(g, r) * rec];
          }
          return v;
        };
        int o_t = 0, o_n = P0;   // off(t), off(t + 1)
        V4 pz = wave < (P0 >> 4) * ncb ? parked(0, wave) : zero4;
        for (int t = 0; t < Tk; ++t) {
          const bool more = t + 1 < Tk;
          const int o_nn = more ? off[t + 2] : o_n, Pn = o_nn - o_n;   // P(t + 1), 0 behind the last step
          const int nblk = ((o_n - o_t) >> 4) * ncb;
          const int cs = t & 1;
          const S* sc = ch0 + cs * blk;
          S* sn = ch0 + (cs ^ 1) * blk;
          V4 pn = zero4;
          if (wave < (Pn >> 4) * ncb) pn = parked(o_n, wave);   // the next step's parked block, off its chain
          for (int it = wave; it < nblk; it += NW) {
            const int qb = it / ncb, cb = it - qb * ncb, j = cb * 16 + c;
            V4 acc = it == wave ? pz : parked(o_t, it);
            const S* arow = sc + (qb * 16 + c) * hs;
            const S* bcol = WSk + j;
#pragma unroll 4
            for (int k = g; k < n4; k += 4) acc = mb_mfma(arow[k], bcol[k * ld], acc);
            if (j < n4) {
              const S bj = j < n ? bb[j] : S(0);
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                const int q = qb * 16 + mb_row<S>(g, r);
                S z = acc[r] + bj, ns = dm::act(sk, z);
                if (j >= n) { z = S(0); ns = S(0); }
                sn[q * hs + j] = ns;
                if (q < Pn) tape[(long)(o_n + q) * rec + os + j] = ns;   // S_{t+1}, where the slot has a step t + 1
                tape[(long)(o_t + q) * rec + odz + j] = z;
              }
            }
          }
          lds_barrier();
          pz = pn;
          o_t = o_n; o_n = o_nn;
        }
      }
      __syncthreads();
      if (!last) {   // hidden_act(z) of all rows: the next layer's input rows
        for (long e = tid; e < R * n4; e += TH) {
          const long r = e / n4;
          const int j = (int)(e - r * n4);
          S* const rt = tape + r * rec;
          rt[onx + j] = j < n ? dm::act(hk, rt[odz + j]) : S(0);
        }
        __syncthreads();
      }
    }
    // ---- the head, a wave a row, all rows at once: z_L on the tape becomes dz_L in place; losses ---------------------------
    // (rnn_minibatch.hip's head; a padding row's dz is zero)
    for (long r = wave; r < R; r += NW) {
      const int t = bt[r >> 4], q = (int)(r - off[t]);
      S* const zr = tape + r * rec + a.t_dz[L - 1];
      if (!runs(q, t)) {
        for (int j = lane; j < nL; j += 64) zr[j] = S(0);
        continue;
      }
      const S* yr = a.Y + ((long)t_seq[k0 + q] * T + t) * nL;
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
        if (lane == 0) a.losses[(long)t_pos[k0 + q] * T + t] = l;
      }
    }
    __syncthreads();
    // ---- backward -----------------------------------------------------------------------------------------------------
    for (int l = L - 1; l >= 0; --l) {
      const int m = a.n[l], n = a.n[l + 1], ld = a.ld[l], sk = a.sk[l];
      const int m4 = (m + 3) & ~3, n4 = (n + 3) & ~3, ncb = (n + 15) >> 4;
      const S* Wk = lds + a.w_off[l];
      const int odz = a.t_dz[l];
      if (sk >= 0) {   // dz_t += (dz_{t+1} W') (.) state_act'(S_{t+1}) on the rows that have a step t + 1, serial in t; then gs
        const S* WSk = lds + a.ws_off[l];
        const int os = a.t_s[l];
        {   // the dz block of the last step: its P(Tk - 1) rows
          const int o_l = off[Tk - 1], Pl = (int)R - o_l;
          for (int e = tid; e < Pl * hs; e += TH) {
            const int q = e / hs, j = e - q * hs;
            ch0[e] = j < n4 ? tape[(long)(o_l + q) * rec + odz + j] : S(0);
          }
        }
        // what step t's block `it` adds to: the cotangent from above G_t and, below P(t + 1), S_{t+1} (o_t, o_n: off(t), off(t + 1))
        auto pre = [&](int o_t, int o_n, int Pn, int it, V4& g0, V4& s1) {
          const int qb = it / ncb, kk = (it - qb * ncb) * 16 + c;
          g0 = zero4; s1 = zero4;
          if (kk < n4) {
            const S* p = tape + (long)(o_t + qb * 16) * rec + odz + kk;
            const S* pn = tape + (long)(o_n + qb * 16) * rec + os + kk;
            const bool carry = qb * 16 < Pn;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              g0[r] = p[mb_row<S>(g, r) * rec];
              if (carry) s1[r] = pn[mb_row<S>(g, r) * rec];
            }
          }
        };
        V4 g0 = zero4, s1 = zero4;
        if (Tk > 1 && wave < ((off[Tk - 1] - off[Tk - 2]) >> 4) * ncb)
          pre(off[Tk - 2], off[Tk - 1], (int)R - off[Tk - 1], wave, g0, s1);
        __syncthreads();
        int cur = 0;
        for (int t = Tk - 2; t >= 0; --t) {
          const int o_t = off[t], o_n = off[t + 1], Pt = o_n - o_t, Pn = off[t + 2] - o_n, nblk = (Pt >> 4) * ncb;
          const S* dcur = ch0 + cur * blk;
          S* dnxt = ch0 + (cur ^ 1) * blk;
          V4 g0n = zero4, s1n = zero4;
          if (t > 0 && wave < ((o_t - off[t - 1]) >> 4) * ncb) pre(off[t - 1], o_t, Pt, wave, g0n, s1n);   // step t - 1's, off its chain
          for (int it = wave; it < nblk; it += NW) {
            const int qb = it / ncb, cb = it - qb * ncb, kk = cb * 16 + c;
            V4 gg = g0, ss = s1;
            if (it != wave) pre(o_t, o_n, Pn, it, gg, ss);
            const bool inb = kk < n4, carry = qb * 16 < Pn;   // (carry: the same for the whole wave)
            V4 acc = zero4;
            if (carry) {
              const S* arow = dcur + (qb * 16 + c) * hs;
              const S* brow = WSk + kk * ld;
#pragma unroll 4
              for (int j = g; j < n4; j += 4) acc = mb_mfma(arow[j], inb ? brow[j] : S(0), acc);
            }
            if (inb) {
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                const int q = qb * 16 + mb_row<S>(g, r);
                S d = S(0);
                if (kk < n) d = carry ? gg[r] + acc[r] * dm::dact(sk, ss[r]) : gg[r];
                dnxt[q * hs + kk] = d;
                tape[(long)(o_t + q) * rec + odz + kk] = d;
              }
            }
          }
          lds_barrier();
          g0 = g0n; s1 = s1n;
          cur ^= 1;
        }
        {   // gs: the rows of dz_0 in ascending order, then the product with W'
          const S* dcur = ch0 + cur * blk;
          S* dsum = ch0 + (cur ^ 1) * blk;
          for (int j = tid; j < n; j += TH) {
            S v = S(0);
            for (int q = 0; q < P0; ++q) v += dcur[q * hs + j];
            dsum[j] = v;
          }
          __syncthreads();
          for (int k = tid; k < n; k += TH) {
            const S* vk = WSk + k * ld;
            S acc = S(0);
#pragma unroll 8
            for (int j = 0; j < n; ++j) acc = dm::fma(vk[j], dsum[j], acc);
            lds[a.s_off[l] + k] -= a.rate_state * acc;
          }
        }
        __syncthreads();
      }
      if (l > 0) {   // dz_{l-1}[r][k] = (dz[r] W)[k] hidden_act'(a_{l-1}[r][k]): time-independent, all R rows as tiles
        const int oin = a.t_in[l], odn = a.t_dz[l - 1], nkb = (m + 15) >> 4;
        const long ntile = (R >> 4) * nkb;
        for (long it = wave; it < ntile; it += NW) {
          const long rb = it / nkb;
          const int kk = (int)(it - rb * nkb) * 16 + c;
          const S* arow = tape + (rb * 16 + c) * rec + odz;
          const S* brow = Wk + kk * ld;
          const bool inb = kk < m4;
          V4 acc = zero4;
#pragma unroll 4
          for (int j = g; j < n4; j += 4) acc = mb_mfma(arow[j], inb ? brow[j] : S(0), acc);
          if (inb) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              S* const rt = tape + (rb * 16 + mb_row<S>(g, r)) * rec;
              rt[odn + kk] = kk < m ? acc[r] * dm::dact(hk, rt[oin + kk]) : S(0);
            }
          }
        }
        __syncthreads();
      }
    }
    // ---- update: every read of the old parameters is behind a barrier above ---------------------------------------------
    for (int l = 0; l < L; ++l) {
      const int m = a.n[l], n = a.n[l + 1], ld = a.ld[l];
      const int odz = a.t_dz[l];
      mb_update<S>(tape, rec, R, a.t_in[l], odz, m, n, ld, lds + a.w_off[l], a.rate_params, wave, c, g);
      if (a.sk[l] >= 0) mb_update<S>(tape, rec, R, a.t_s[l], odz, n, n, ld, lds + a.ws_off[l], a.rate_params, wave, c, g);
      for (int j = tid; j < n; j += TH) {
        const S* p = tape;
        S gb = S(0);
        for (long r = 0; r < R; r += 16, p += 16 * rec) {   // R is a multiple of 16: 16 loads in flight, the sum in row order
          S v[16];
#pragma unroll
          for (int u = 0; u < 16; ++u) v[u] = p[u * rec + odz + j];
#pragma unroll
          for (int u = 0; u < 16; ++u) gb += v[u];
        }
        lds[a.b_off[l] + j] -= a.rate_params * gb;
      }
    }
    __syncthreads();
  }
  mb_stack_out(a, lds, tid);
}

template <class S>
void go_minibatch_ragged(const RnnMinibatchPlan& p, const RnnMinibatchOperands& o, const int* tab, hipStream_t s) {
  static bool attr = false;
  if (!attr) {
    TO_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(rnn_minibatch_ragged_kernel<S>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)GEN_LDS_MAX));
    attr = true;
  }
  launch_k(rnn_minibatch_ragged_kernel<S>, dim3(1), dim3(MB_THREADS), p.lds, s, mb_args<S>(p, o), tab);
}

}  // namespace

// The schedule of a call: per minibatch its members sorted by length (descending, stable), per step the first row of its
// packed block.  tab: seq[n_idx], pos[n_idx], len[n_idx] by slot position k M + q; {Tk, where off begins} per minibatch; then
// per minibatch off[0 .. Tk] and, one entry per 16 rows, the step a row block belongs to.
bool rnn_minibatch_ragged_schedule(int64_t M, int64_t n_idx, const int64_t* idx, const int64_t* lens, std::vector<int>* tab,
                                   int64_t* max_rows) {
  const int64_t n_steps = (n_idx + M - 1) / M;
  int64_t words = 3 * n_idx + 2 * n_steps;
  std::vector<int64_t> order((size_t)M);
  tab->assign((size_t)words, 0);
  *max_rows = 0;
  for (int64_t k = 0; k < n_steps; ++k) {
    const int64_t k0 = k * M, sz = std::min(M, n_idx - k0);
    auto len_of = [&](int64_t j) { return lens[idx ? idx[j] : j]; };
    std::iota(order.begin(), order.begin() + sz, k0);
    std::stable_sort(order.begin(), order.begin() + sz, [&](int64_t x, int64_t y) { return len_of(x) > len_of(y); });
    const int64_t Tk = len_of(order[0]);
    int64_t rows = 0, act = sz;
    for (int64_t t = 0; t < Tk; ++t) {   // act(t): the slots whose length is above t
      while (len_of(order[act - 1]) <= t) --act;
      rows += (act + 15) & ~int64_t(15);
    }
    if (words + Tk + 1 + rows / 16 > 2147483647LL) return false;
    tab->resize((size_t)(words + Tk + 1 + rows / 16));
    int* const T0 = tab->data();
    for (int64_t q = 0; q < sz; ++q) {
      const int64_t j = order[q], seq = idx ? idx[j] : j;
      if (seq > 2147483647LL) return false;
      T0[k0 + q] = (int)seq;
      T0[n_idx + k0 + q] = (int)j;
      T0[2 * n_idx + k0 + q] = (int)lens[seq];
    }
    T0[3 * n_idx + 2 * k] = (int)Tk;
    T0[3 * n_idx + 2 * k + 1] = (int)words;
    int *off = T0 + words, *bt = off + Tk + 1;
    off[0] = 0;
    act = sz;
    for (int64_t t = 0; t < Tk; ++t) {
      while (len_of(order[act - 1]) <= t) --act;
      const int P = (int)((act + 15) & ~int64_t(15));
      off[t + 1] = off[t] + P;
      for (int rb = off[t] / 16; rb < off[t + 1] / 16; ++rb) bt[rb] = (int)t;
    }
    words += Tk + 1 + rows / 16;
    *max_rows = std::max(*max_rows, rows);
  }
  return true;
}

// o.idx is not read (the tables name the sequences); o.tape holds max_rows * p.rec elements
void launch_rnn_minibatch_ragged(int dtype, const RnnMinibatchPlan& p, const RnnMinibatchOperands& o, const int* tab,
                                 hipStream_t s) {
  TO_CHECK(o.L >= 1 && o.L <= RNN_GEN_MAX_LAYERS && o.n_idx >= 1 && o.T >= 1 && o.M >= 1 && o.M <= p.Mp && p.lds <= GEN_LDS_MAX &&
               o.tape != nullptr && tab != nullptr, TO_ERR_STATE, "internal: rnn_minibatch_ragged outside its plan");
  if (dtype == TO_F64) go_minibatch_ragged<double>(p, o, tab, s);
  else go_minibatch_ragged<float>(p, o, tab, s);
  TO_HIP(hipGetLastError());
  count_launch();
}

}  // namespace to
