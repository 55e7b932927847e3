// Minibatch training of a recurrent stack (to_rnn_stack_minibatch_sgd, route B): every update of a call -- forward over T
// steps, BPTT, the update, M sequences an update -- as ONE launch by ONE workgroup on 16 x 16 x 4 matrix instructions
// (v_mfma_f32_16x16x4_f32 / v_mfma_f64_16x16x4_f64: the fragment shapes are the same, so one template serves both types).  The
// updates are a dependent chain, so there is nothing to spread over workgroups and nothing crosses one: no spin, no flag, no
// residency requirement; the kernel waits on nothing but its own barriers.
//   Rows              : inside an update row r = t * Mp + q, time-major, Mp = M rounded up to 16: a step's rows are Mp / 16
//                       whole MFMA row blocks.  Rows q >= the minibatch's size (M no multiple of 16, the short last minibatch)
//                       are padding: their input is zero, their dz is forced to zero behind the head, so they add exactly +0
//                       to every gradient and to gs; they are never read from X / Y and never written to losses.
//   LDS               : for the whole call every layer's W, W' and b and the learned initial states (loaded once, written back
//                       once).  Matrices are k-major M[k][j], zero-padded to a multiple of 4 in k and of 16 in j, the leading
//                       dimension the next value above that which is 17 (mod 32).  The forward's B fragment reads 16
//                       consecutive columns at each of 4 consecutive k (addresses 17 g + c, g < 4, c < 16, in fp32 words),
//                       the backward's (dz W, dz W') one column index at 16 consecutive k, a leading dimension apart
//                       (17 c + g): neither collapses onto one bank, as rnn_online.hip's n | 1 does for its two.  Then the
//                       chain blocks: [2][Mp][hs], hs = the widest stateful layer rounded up to 16, plus 4 -- the forward
//                       recurrence's state block, ping-pong, and afterwards the backward recurrence's dz block, ping-pong.
//   The tape          : per row one record -- every layer's input row, every stateful layer's S_t (S_0 = s) and every layer's
//                       z_t, later dz_t -- every field padded to four elements (16 bytes in fp32) with zeros that every
//                       writer of a field writes.  A pool buffer in global memory that only this workgroup touches, written
//                       and then read back behind a barrier; T does not bound the range.  (A tape in LDS is not built.)
//   How it is looped  : rnn_online_kernel's layer-major loops.  Forward, layer l: the input part of all T Mp rows as MFMA
//                       tiles dealt to the waves (A fragments from the tape, B from LDS); parked on the tape they are the
//                       recurrence's accumulator INITIAL VALUES.  The recurrence, serial in t: per step the (Mp / 16) x
//                       (Hp / 16) output blocks are dealt to the waves; a wave picks its parked block up as the accumulator,
//                       runs Hp / 4 MFMAs over the state block in LDS, adds the bias, applies state_act and stores the new
//                       state block to the other LDS buffer and to the tape -- ONE LDS-only barrier a step, the next step's
//                       parked block of a wave's first output block loaded ahead of this step's chain.  hidden_act of all
//                       rows comes last.  The head: loss_grad_rows_kernel's formulas on z_L, a wave a row, all rows at once.
//                       Backward, layer L-1 down to 0: dz_t += (dz_{t+1} W') (.) state_act'(S_{t+1}) serial in t in the same
//                       way, then gs (the rows of dz_0 summed in ascending row order, then one product with W'), then the
//                       cotangent of the layer below for all rows as tiles.  Update, behind one barrier after the last read
//                       of the old parameters: g[k][j] = sum_r in[r][k] dz[r][j] is an MFMA product whose reduction dimension
//                       is the row, r ascending in steps of 4; 16 x 16 output blocks are dealt to the waves and M[k][j] -= rate
//                       g goes from the accumulator fragment straight into LDS.  Bias sums in ascending row order.
//   Determinism       : every sum's order is fixed by (dtype, widths, M) alone: a repeated call gives the same bits, and so
//                       does a call cut at a minibatch boundary into two.
// MB_THREADS = 512, eight waves: fp32 70 -> 130 -> 3 at M = 16 has nine output blocks a step.  Not measured against 256.
// The workgroup's shape, the MFMA block, the kernel's arguments and the update's row reduction are rnn_minibatch_dev.hpp's,
// shared with rnn_minibatch_ragged.hip.
#include <algorithm>

#include "rnn_minibatch_dev.hpp"

namespace to {

namespace {

template <class S>
__global__ __launch_bounds__(MB_THREADS) void rnn_minibatch_kernel(RnnMinibatchArgs<S> a) {
  extern __shared__ __align__(16) unsigned char minibatch_lds[];
  S* const lds = reinterpret_cast<S*>(minibatch_lds);
  using V4 = mb_v4<S>;
  constexpr int TH = MB_THREADS, NW = MB_NW;
  const int L = a.L, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 15, g = lane >> 4, hk = a.hidden_kind;
  const int n0 = a.n[0], nL = a.n[L], Mp = a.Mp, hs = a.hs, blk = Mp * hs, qbs = Mp >> 4;
  const long T = a.T, rec = a.rec, R = T * Mp, step = (long)Mp * rec;   // step: one time step's records
  S* const tape = a.tape;
  S* const ch0 = lds + a.chain_off;
  const V4 zero4 = {S(0), S(0), S(0), S(0)};
  // ---- the parameters and the initial states, once: zeros everywhere, then the values -----------------------------------
  for (int e = tid; e < a.chain_off; e += TH) lds[e] = S(0);
  __syncthreads();
  for (int l = 0; l < L; ++l) {
    const int m = a.n[l], n = a.n[l + 1], ld = a.ld[l];
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
  __syncthreads();

  for (long k0 = 0; k0 < a.n_idx; k0 += a.M) {
    const int sz = (int)min(a.M, a.n_idx - k0);   // the minibatch's sequences: rows q < sz of every step
    // ---- the rows of X onto the tape (padding rows: zeros); S_0 = s in every row of step 0 ---------------------------------
    {
      const int w0 = (n0 + 3) & ~3, o0 = a.t_in[0];
      for (long e = tid; e < R * w0; e += TH) {
        const long r = e / w0, t = r / Mp;
        const int j = (int)(e - r * w0), q = (int)(r - t * Mp);
        S v = S(0);
        if (q < sz && j < n0) {
          const long seq = a.idx ? (long)a.idx[k0 + q] : k0 + q;
          v = a.X[(seq * T + t) * n0 + j];
        }
        tape[r * rec + o0 + j] = v;
      }
    }
    for (int l = 0; l < L; ++l) {
      if (a.sk[l] < 0) continue;
      const int n = a.n[l + 1], n4 = (n + 3) & ~3;
      for (int e = tid; e < Mp * n4; e += TH) {
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
      // the input parts of all rows (a stateless layer: all of z, and what comes behind it)
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
      // the recurrence: z_t = (parked block) + S_t W'^T + b, S_{t+1} = state_act(z_t)
      {
        const S* WSk = lds + a.ws_off[l];
        const int os = a.t_s[l], nblk = qbs * ncb;
        auto parked = [&](long t, int it) {
          const int qb = it / ncb, j = (it - qb * ncb) * 16 + c;
          V4 v = zero4;
          if (j < n4) {
            const S* p = tape + t * step + (long)(qb * 16) * rec + odz + j;
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = p[mb_row<S>(g, r) * rec];
          }
          return v;
        };
        V4 pz = wave < nblk ? parked(0, wave) : zero4;
        for (long t = 0; t < T; ++t) {
          const bool more = t + 1 < T;
          const int cs = (int)(t & 1);
          const S* sc = ch0 + cs * blk;
          S* sn = ch0 + (cs ^ 1) * blk;
          V4 pn = zero4;
          if (more && wave < nblk) pn = parked(t + 1, wave);   // the next step's parked block, off its chain
          for (int it = wave; it < nblk; it += NW) {
            const int qb = it / ncb, cb = it - qb * ncb, j = cb * 16 + c;
            V4 acc = it == wave ? pz : parked(t, it);
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
                S* const rt = tape + t * step + q * rec;
                sn[q * hs + j] = ns;
                if (more) rt[step + os + j] = ns;   // S_{t+1}
                rt[odz + j] = z;
              }
            }
          }
          lds_barrier();
          pz = pn;
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
    // (loss_grad_rows_kernel's formulas; a lane reads and writes its own elements only; a padding row's dz is zero)
    for (long r = wave; r < R; r += NW) {
      const long t = r / Mp;
      const int q = (int)(r - t * Mp);
      S* const zr = tape + r * rec + a.t_dz[L - 1];
      if (q >= sz) {
        for (int j = lane; j < nL; j += 64) zr[j] = S(0);
        continue;
      }
      const long seq = a.idx ? (long)a.idx[k0 + q] : k0 + q;
      const S* yr = a.Y + (seq * T + t) * nL;
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
        if (lane == 0) a.losses[(k0 + q) * T + t] = l;
      }
    }
    __syncthreads();
    // ---- backward -----------------------------------------------------------------------------------------------------
    for (int l = L - 1; l >= 0; --l) {
      const int m = a.n[l], n = a.n[l + 1], ld = a.ld[l], sk = a.sk[l];
      const int m4 = (m + 3) & ~3, n4 = (n + 3) & ~3, ncb = (n + 15) >> 4;
      const S* Wk = lds + a.w_off[l];
      const int odz = a.t_dz[l];
      if (sk >= 0) {   // dz_t += (dz_{t+1} W') (.) state_act'(S_{t+1}), serial in t; then s -= rate_state (sum_q dz_0[q]) W'
        const S* WSk = lds + a.ws_off[l];
        const int os = a.t_s[l], nblk = qbs * ncb;
        for (int e = tid; e < blk; e += TH) {   // the dz block of the last step
          const int q = e / hs, j = e - q * hs;
          ch0[e] = j < n4 ? tape[(T - 1) * step + q * rec + odz + j] : S(0);
        }
        // what step t's block `it` adds to: the cotangent from above G_t and S_{t+1}
        auto pre = [&](long t, int it, V4& g0, V4& s1) {
          const int qb = it / ncb, kk = (it - qb * ncb) * 16 + c;
          g0 = zero4; s1 = zero4;
          if (kk < n4) {
            const S* p = tape + t * step + (long)(qb * 16) * rec;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const S* pr = p + mb_row<S>(g, r) * rec;
              g0[r] = pr[odz + kk];
              s1[r] = pr[step + os + kk];
            }
          }
        };
        V4 g0 = zero4, s1 = zero4;
        if (T > 1 && wave < nblk) pre(T - 2, wave, g0, s1);
        __syncthreads();
        int cur = 0;
        for (long t = T - 2; t >= 0; --t) {
          const S* dcur = ch0 + cur * blk;
          S* dnxt = ch0 + (cur ^ 1) * blk;
          V4 g0n = zero4, s1n = zero4;
          if (t > 0 && wave < nblk) pre(t - 1, wave, g0n, s1n);   // step t - 1's reads, off its chain
          for (int it = wave; it < nblk; it += NW) {
            const int qb = it / ncb, cb = it - qb * ncb, kk = cb * 16 + c;
            V4 gg = g0, ss = s1;
            if (it != wave) pre(t, it, gg, ss);
            const S* arow = dcur + (qb * 16 + c) * hs;
            const S* brow = WSk + kk * ld;
            const bool inb = kk < n4;
            V4 acc = zero4;
#pragma unroll 4
            for (int j = g; j < n4; j += 4) acc = mb_mfma(arow[j], inb ? brow[j] : S(0), acc);
            if (inb) {
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                const int q = qb * 16 + mb_row<S>(g, r);
                const S d = kk < n ? gg[r] + acc[r] * dm::dact(sk, ss[r]) : S(0);
                dnxt[q * hs + kk] = d;
                tape[t * step + q * rec + odz + kk] = d;
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
            for (int q = 0; q < Mp; ++q) v += dcur[q * hs + j];
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
      if (l > 0) {   // dz_{l-1}[r][k] = (dz[r] W)[k] hidden_act'(a_{l-1}[r][k]): time-independent, all rows as tiles
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
  // ---- the parameters and the initial states back, once ----------------------------------------------------------------
  for (int l = 0; l < L; ++l) {
    const int m = a.n[l], n = a.n[l + 1], ld = a.ld[l];
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

template <class S>
void go_minibatch(const RnnMinibatchPlan& p, const RnnMinibatchOperands& o, hipStream_t s) {
  static bool attr = false;
  if (!attr) {
    TO_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(rnn_minibatch_kernel<S>), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)GEN_LDS_MAX));
    attr = true;
  }
  launch_k(rnn_minibatch_kernel<S>, dim3(1), dim3(MB_THREADS), p.lds, s, mb_args<S>(p, o));
}

}  // namespace

// The LDS of the one workgroup, in elements: per layer W [up4(m)][ld], W' [up4(n)][ld] and s [up4(n)] (stateful), b [up4(n)],
// ld the next value above n rounded up to 16 that is 17 (mod 32); then the two chain blocks [Mp][hs].  The tape record: per
// layer the input row, S_t (stateful) and z_t / dz_t, each padded to four elements.  The plan fails when all that exceeds the
// limit: T never decides that.
bool rnn_minibatch_plan(int dtype, int L, const int64_t* widths, const int* stateful, int64_t M, int64_t T, RnnMinibatchPlan* p) {
  if (L < 1 || L > RNN_GEN_MAX_LAYERS || M < 1 || M > RNN_MINIBATCH_MAX_M || T < 1) return false;
  for (int l = 0; l <= L; ++l)
    if (widths[l] < 1 || widths[l] > 65536) return false;
  const int64_t es = dtype == TO_F64 ? 8 : 4, cap = (int64_t)GEN_LDS_MAX / es;
  int64_t off = 0, rec = 0, ws = 0;
  auto up4 = [](int64_t v) { return (v + 3) & ~int64_t(3); };
  auto up16 = [](int64_t v) { return (v + 15) & ~int64_t(15); };
  for (int l = 0; l < L; ++l) {
    const int64_t m = widths[l], n = widths[l + 1], n16 = up16(n), ld = n16 + ((n16 & 16) ? 1 : 17);
    p->ld[l] = (int)ld;
    p->w_off[l] = (int)off; off += up4(m) * ld;
    if (off > cap) return false;
    p->ws_off[l] = (int)off;
    if (stateful[l]) off += up4(n) * ld;
    if (off > cap) return false;
    p->b_off[l] = (int)off; off += up4(n);
    p->s_off[l] = (int)off;
    if (stateful[l]) off += up4(n);
    p->t_in[l] = (int)rec; rec += up4(m);
    p->t_s[l] = (int)rec;
    if (stateful[l]) { rec += up4(n); ws = std::max(ws, n); }
    p->t_dz[l] = (int)rec; rec += up4(n);
  }
  p->Mp = (int)up16(M);
  p->hs = (int)(up16(ws) + 4);
  p->chain_off = (int)off;
  off += 2 * (int64_t)p->Mp * p->hs;
  if (off > cap) return false;
  if (rec % 32 == 0) rec += 4;   // (the rows of a block not all in one channel)
  if (T > 2147483647LL / p->Mp) return false;   // (more than 2^31-1 rows: refused by every route)
  p->rec = rec;
  p->tape_elems = T * p->Mp * rec;
  p->lds = (size_t)(off * es);
  return true;
}

void launch_rnn_minibatch(int dtype, const RnnMinibatchPlan& p, const RnnMinibatchOperands& o, hipStream_t s) {
  TO_CHECK(o.L >= 1 && o.L <= RNN_GEN_MAX_LAYERS && o.n_idx >= 1 && o.T >= 1 && o.M >= 1 && o.M <= p.Mp && p.lds <= GEN_LDS_MAX &&
               o.tape != nullptr, TO_ERR_STATE, "internal: rnn_minibatch outside its plan");
  if (dtype == TO_F64) go_minibatch<double>(p, o, s);
  else go_minibatch<float>(p, o, s);
  TO_HIP(hipGetLastError());
  count_launch();
}

}  // namespace to
