// The recurrence of a `fullyConnected` layer (Recurrent.hs:91-119) over a whole sequence, for to_rnn_stack_*.  Everything
// of BPTT that does not depend on time (input projections, heads, weight gradients, input cotangents) is one GEMM over all
// B*T rows in stack_rnn.cpp; what is left is a chain of T dependent [rows, H] x [H, H] products:
//   forward  z_t  = P_t + s_{t-1} W'^T,  s_t = act(z_t)                   (P_t: the input projection, z_t in place over it)
//   reverse  dz_t = G_t + (dz_{t+1} W') (.) act'(s_t),  dz_T = 0          (G_t: the output-path cotangent, in place)
// act: the layer's state activation, a template parameter of the kernel (ACT_KIND_LOGISTIC: s (1 - s); ACT_KIND_TANH:
// tanh, 1 - s^2 -- devmath.hpp).
// Both are out_t[j] = epilogue(sum_k v_{t-1}[k] M[k][j]) with M = W'^T (forward, a transposed copy) or W' (reverse), so one
// kernel serves both.  rnn_seq_kernel: ONE launch per layer and direction covers all T steps.  Each workgroup owns R
// whole sequences (rows) and all H columns, so a step's new vector never leaves the workgroup: it is exchanged through
// LDS (double-buffered, one barrier per step) -- no inter-workgroup hand-over, no spin, no residency requirement, any grid
// size.  M sits in LDS when it fits beside the two state buffers (up to H = 201 in fp32, 142 in fp64) and is read through
// L1 / L2 otherwise -- which loses to the per-step route (profiles/r07_rnn_scan.txt): stack_rnn.cpp routes only the LDS form
// automatically.  The next step's P_t / G_t values are loaded before the barrier.  Every sum has a fixed order.
// Layouts (stack_rnn.cpp, time-major): Z [T][B][H], St [T+1][B][H] with row block 0 = the initial states.
#include <algorithm>

#include "common.hpp"
#include "devmath.hpp"

namespace to {

namespace {

constexpr int RNN_THREADS = 256;
constexpr int RNN_QMAX = RNN_SEQ_MAX_H / RNN_THREADS;  // (row, column) items per thread: R * H <= RNN_SEQ_MAX_H
constexpr size_t RNN_LDS_MAX = 160 * 1024;

template <class S>
struct RnnSeqArgs {
  const S* M;  // [H][H]: out[j] = sum_k v[k] M[k][j]
  S* Z;        // [T][B][H]: forward P -> z, reverse G -> dz, in place
  S* St;       // [T+1][B][H]: forward writes blocks 1..T from block 0; reverse reads blocks 1..T
  long B, T;
  int H, R;
};

template <class S, bool REV, bool MLDS, int ACT>
__global__ __launch_bounds__(RNN_THREADS) void rnn_seq_kernel(RnnSeqArgs<S> a) {
  extern __shared__ __align__(16) unsigned char rnn_lds[];
  const int H = a.H, R = a.R;
  S* v = reinterpret_cast<S*>(rnn_lds);  // [2][R][H]
  S* Ml = v + 2 * (size_t)R * H;         // [H][H] (MLDS)
  const long b0 = (long)blockIdx.x * R;
  const int rows = (int)min((long)R, a.B - b0);
  const int items = rows * H;
  const int tid = threadIdx.x;
  const long blk = a.B * (long)H;  // one time step of Z / St
  if (MLDS)
    for (int e = tid; e < H * H; e += RNN_THREADS) Ml[e] = a.M[e];
  const S* M = MLDS ? Ml : a.M;
  // v_{-1}: the initial states (forward) or dz_T = 0 (reverse)
  for (int e = tid; e < items; e += RNN_THREADS) v[e] = REV ? S(0) : a.St[b0 * H + e];
  int rq[RNN_QMAX], jq[RNN_QMAX];
  S pre[RNN_QMAX];
#pragma unroll
  for (int q = 0; q < RNN_QMAX; ++q) {
    const int item = tid + q * RNN_THREADS;
    rq[q] = item / H;
    jq[q] = item - rq[q] * H;
    const long t0 = REV ? a.T - 1 : 0;
    pre[q] = item < items ? a.Z[t0 * blk + (b0 + rq[q]) * H + jq[q]] : S(0);
  }
  __syncthreads();
  int cur = 0;
  for (long step = 0; step < a.T; ++step) {
    const long t = REV ? a.T - 1 - step : step;
    const S* vc = v + (size_t)cur * R * H;
    S* vn = v + (size_t)(cur ^ 1) * R * H;
#pragma unroll
    for (int q = 0; q < RNN_QMAX; ++q) {
      const int item = tid + q * RNN_THREADS;
      if (item < items) {
        const int r = rq[q], j = jq[q];
        const long off = t * blk + (b0 + r) * H + j;
        S acc = S(0);
        if (!REV || step > 0) {
          const S* vr = vc + (size_t)r * H;
          const S* mj = M + j;
#pragma unroll 4
          for (int k = 0; k < H; ++k) acc = dm::fma(vr[k], mj[(size_t)k * H], acc);
        }
        S o;
        if (!REV) {
          const S z = pre[q] + acc;
          a.Z[off] = z;
          if constexpr (ACT == ACT_KIND_TANH) o = dm::tanh_act(z);
          else o = dm::logistic(z);
          a.St[off + blk] = o;
        } else {
          const S h = a.St[off + blk];
          if constexpr (ACT == ACT_KIND_TANH) o = dm::fma(acc, dm::tanh_dact(h), pre[q]);
          else o = dm::fma(acc * h, S(1) - h, pre[q]);
          a.Z[off] = o;
        }
        vn[item] = o;
        const long tn = REV ? t - 1 : t + 1;  // the next step's addend, loaded under the barrier
        if (tn >= 0 && tn < a.T) pre[q] = a.Z[off + (tn - t) * blk];
      }
    }
    __syncthreads();
    cur ^= 1;
  }
}

template <class S, bool REV, bool MLDS, int ACT>
void go(const RnnSeqPlan& p, const void* M, void* Z, void* St, int64_t B, int64_t T, int64_t H, hipStream_t s) {
  static bool attr = false;
  if (!attr) {
    TO_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(rnn_seq_kernel<S, REV, MLDS, ACT>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)RNN_LDS_MAX));
    attr = true;
  }
  RnnSeqArgs<S> a{(const S*)M, (S*)Z, (S*)St, (long)B, (long)T, (int)H, p.R};
  launch_k(rnn_seq_kernel<S, REV, MLDS, ACT>, dim3((unsigned)p.grid), dim3(RNN_THREADS), p.lds, s, a);
}

}  // namespace

// R rows per workgroup: enough rows to give every thread an item (R * H >= 256), more when the batch would need more than
// 256 workgroups, never more than RNN_SEQ_MAX_H items.  M in LDS when it fits beside the two state vectors.
bool rnn_seq_plan(int dtype, int64_t H, int64_t B, RnnSeqPlan* p) {
  if (H < 1 || H > RNN_SEQ_MAX_H || B < 1) return false;
  const int64_t es = dtype == TO_F64 ? 8 : 4;
  const int64_t rmax = RNN_SEQ_MAX_H / H;
  int64_t R = std::max<int64_t>(1, RNN_THREADS / H);
  R = std::max(R, (B + 255) / 256);
  R = std::min({R, rmax, B});
  p->R = (int)R;
  p->grid = (B + R - 1) / R;
  const size_t vec = (size_t)(2 * R * H * es);
  p->m_lds = vec + (size_t)(H * H * es) <= RNN_LDS_MAX;
  p->lds = vec + (p->m_lds ? (size_t)(H * H * es) : 0);
  return p->grid <= 2147483647LL;
}

template <class S, bool REV, bool MLDS>
static void go_act(int act_kind, const RnnSeqPlan& p, const void* M, void* Z, void* St, int64_t B, int64_t T, int64_t H,
                   hipStream_t s) {
  if (act_kind == ACT_KIND_TANH) go<S, REV, MLDS, ACT_KIND_TANH>(p, M, Z, St, B, T, H, s);
  else go<S, REV, MLDS, ACT_KIND_LOGISTIC>(p, M, Z, St, B, T, H, s);
}

void launch_rnn_seq(int dtype, bool reverse, const RnnSeqPlan& p, const void* M, void* Z, void* St, int64_t B, int64_t T,
                    int64_t H, int act_kind, hipStream_t s) {
  if (B == 0 || T == 0) return;
  TO_CHECK(act_kind == ACT_KIND_LOGISTIC || act_kind == ACT_KIND_TANH, TO_ERR_ARG, "rnn_seq: unknown state activation");
  const int k = act_kind;
  if (dtype == TO_F64) {
    if (reverse) p.m_lds ? go_act<double, true, true>(k, p, M, Z, St, B, T, H, s) : go_act<double, true, false>(k, p, M, Z, St, B, T, H, s);
    else p.m_lds ? go_act<double, false, true>(k, p, M, Z, St, B, T, H, s) : go_act<double, false, false>(k, p, M, Z, St, B, T, H, s);
  } else {
    if (reverse) p.m_lds ? go_act<float, true, true>(k, p, M, Z, St, B, T, H, s) : go_act<float, true, false>(k, p, M, Z, St, B, T, H, s);
    else p.m_lds ? go_act<float, false, true>(k, p, M, Z, St, B, T, H, s) : go_act<float, false, false>(k, p, M, Z, St, B, T, H, s);
  }
  TO_HIP(hipGetLastError());
  count_launch();
}

}  // namespace to
