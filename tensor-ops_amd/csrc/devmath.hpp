// Device-only scalar math of the kernel files: the float / double leaf functions, the logistics, the hidden / state
// activations and the whole-wave folds, ONE definition per distinct function, the name saying which function it is.  Call
// sites write the names qualified (dm::exp): HIP declares global exp(float) and its kin.  Only leaves live here -- an
// expression at a call site keeps its own operation order.  (Kernel source kept in strings for the runtime compiler --
// rowprog.cpp, expr_jit.cpp -- cannot include this and carries its own.)
#pragma once
#include "common.hpp"  // hip_runtime.h, ACT_KIND_*

namespace to {
namespace dm {

// ---- leaves --------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float exp(float x) { return expf(x); }
__device__ __forceinline__ double exp(double x) { return ::exp(x); }
// __expf in fp32: a different function from exp (v_exp_f32 on a scaled argument, no range handling).  fp64 has no fast form:
// the double overload IS exp.
__device__ __forceinline__ float exp_fast(float x) { return __expf(x); }
__device__ __forceinline__ double exp_fast(double x) { return ::exp(x); }
__device__ __forceinline__ float log(float x) { return logf(x); }
__device__ __forceinline__ double log(double x) { return ::log(x); }
__device__ __forceinline__ float tanh(float x) { return tanhf(x); }
__device__ __forceinline__ double tanh(double x) { return ::tanh(x); }
__device__ __forceinline__ float sqrt(float x) { return sqrtf(x); }
__device__ __forceinline__ double sqrt(double x) { return ::sqrt(x); }
__device__ __forceinline__ float abs(float x) { return fabsf(x); }
__device__ __forceinline__ double abs(double x) { return ::fabs(x); }
__device__ __forceinline__ float fma(float a, float b, float c) { return fmaf(a, b, c); }
__device__ __forceinline__ double fma(double a, double b, double c) { return ::fma(a, b, c); }
// fmaxf / fmax: a NaN operand is dropped, the other one returned
__device__ __forceinline__ float max(float a, float b) { return fmaxf(a, b); }
__device__ __forceinline__ double max(double a, double b) { return ::fmax(a, b); }

// ---- the cross-entropy term of every softmax row head ------------------------------------------------------------------
// -t log softmax(z)_j written on d = z_j - max z and lse = log(sum_k exp(z_k - max z)): t * (lse - d).  The same value as
// -t * log(exp(d) / sum) while exp(d) is a normal number, and finite beyond: a row whose logits lie further apart than the
// exponential's range (about 87 in fp32, whose denormal results are flushed, 745 in fp64) has p = 0 there, and 0 * log(0) is
// a NaN.  What stays non-finite is arithmetic: d = -inf under t = 0 (0 * inf), and inf - inf.
template <class S> __device__ __forceinline__ S ce_term(S t, S d, S lse) { return t * (lse - d); }

// ---- logistics: three different functions in fp32 (DESIGN.md 3.3 says which route computes which) -------------------
// exact: libm's exponential and a true division
template <class S> __device__ __forceinline__ S logistic(S x) { return S(1) / (S(1) + exp(-x)); }
// the fast exponential under a true division (fp64: the same function as logistic).  The two persistent per-sample kernels
// (online_sgd.hip, induce_seq.hip) use it: a sample's whole forward and backward pass sits on their dependent chain.
template <class S> __device__ __forceinline__ S logistic_fast(S x) { return S(1) / (S(1) + exp_fast(-x)); }
// the fast exponential under v_rcp_f32 (1 ulp) instead of the division; fp32 only
__device__ __forceinline__ float logistic_rcp(float x) { return __builtin_amdgcn_rcpf(1.0f + __expf(-x)); }

// ---- activations of the one-call stack entries, numbered ACT_KIND_* (common.hpp) --------------------------------------
// The tanh pair -- the value, and the derivative FROM THE STORED OUTPUT h -- is what the GEMM epilogues compute too: every
// route of an entry computes the same tanh.
template <class S> __device__ __forceinline__ S tanh_act(S z) { return tanh(z); }
template <class S> __device__ __forceinline__ S tanh_dact(S h) { return S(1) - h * h; }
// by compile-time kind, on logistic_fast (online_sgd.hip, induce_seq.hip): the value, and `s * act'` written on h
template <int ACT, class S>
__device__ __forceinline__ S hid_act_fast(S z) {
  if constexpr (ACT == ACT_KIND_TANH) return tanh_act(z);
  else return logistic_fast(z);
}
template <int ACT, class S>
__device__ __forceinline__ S hid_dact_fast(S s, S h) {
  if constexpr (ACT == ACT_KIND_TANH) return s * tanh_dact(h);
  else return s * h * (S(1.0) - h);
}
// by run-time kind, on the exact logistic (rnn_generate.hip, rnn_online.hip): the value, and act' written on h
template <class S> __device__ __forceinline__ S act(int kind, S z) { return kind == ACT_KIND_TANH ? tanh_act(z) : logistic(z); }
template <class S> __device__ __forceinline__ S dact(int kind, S h) { return kind == ACT_KIND_TANH ? tanh_dact(h) : h * (S(1) - h); }

// ---- folds over the 64 lanes of a wave: the xor butterfly 32, 16 .. 1, the result in every lane ------------------------
template <class S>
__device__ __forceinline__ S wave_sum(S v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
template <class S>
__device__ __forceinline__ S wave_max(S v) {   // max's NaN rule at every level
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off, 64));
  return v;
}

}  // namespace dm
}  // namespace to
