// What the step's kernels assume about the arguments they take as 32-bit leading scalars, in plain C++ (no HIP): the
// launchers refuse a problem that fails these, and tests/test_step_preload.py compiles this header into a host program of
// its own.
#pragma once
#include <algorithm>
#include <cstdint>

namespace to {

// does the value survive the trip through a 32-bit signed kernel argument?  (launch_gemm_small_pair: the first problem's
// output row stride)
inline bool fits_i32(int64_t v) { return v == (int64_t)(int32_t)v; }

// The kernels form 32-bit byte offsets into A and B, and the forward kernel takes the two image strides (a_sx: a_sm of a
// k-contiguous A, else a_sk; b_sx likewise) as 32-bit leading scalars: the padded span of each operand stays below 2 GiB and
// each image stride fits an int.  Strides are in elements of four bytes.
inline bool t32_spans_fit(int64_t M, int64_t N, int64_t K, int64_t a_sm, int64_t a_sk, int64_t b_sn, int64_t b_sk) {
  for (const int64_t v : {M, N, K, a_sm, a_sk, b_sn, b_sk})
    if (!fits_i32(v)) return false;
  if (M < 0 || N < 0 || K < 0 || M + 32 >= (1LL << 29) || N + 32 >= (1LL << 29) || K >= (1LL << 29)) return false;   // (with a stride of 1 already too long; and the sums below stay inside 64 bits)
  if ((M + 32) * std::max<int64_t>(a_sm, 1) * 4 + K * std::max<int64_t>(a_sk, 1) * 4 >= (1LL << 31)) return false;
  if ((N + 32) * std::max<int64_t>(b_sn, 1) * 4 + K * std::max<int64_t>(b_sk, 1) * 4 >= (1LL << 31)) return false;
  return true;
}

}  // namespace to
