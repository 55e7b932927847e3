// The host side of the single-XCD exchange (xcd_exchange.hpp): the state a kernel file keeps between launches, the
// watchdog's length and the placement probe.
#include <cstdlib>
#include <cstring>

#include "xcd_exchange.hpp"

namespace to {

namespace xe {

void XcdExchange::status_alloc() {
  if (status_) return;
  TO_HIP(hipHostMalloc(&status_, 16, hipHostMallocMapped));
  TO_HIP(hipHostGetDevicePointer(&status_dev_, status_, 0));
  std::memset(status_, 0, 16);
}

void XcdExchange::reserve(size_t bytes) {
  if (with_votes_ && !votes_) TO_HIP(hipMalloc(&votes_, VOTE_BYTES));
  status_alloc();
  if (cap_ < bytes) {
    if (exch_) (void)hipFree(exch_);
    exch_ = nullptr;
    cap_ = 0;
    TO_HIP(hipMalloc(&exch_, bytes));
    cap_ = bytes;
  }
  used_ = bytes;
}

// (no tag or vote of an earlier launch may pass for one of this launch)
void XcdExchange::zero(hipStream_t s) {
  if (with_votes_) TO_HIP(hipMemsetAsync(votes_, 0, VOTE_BYTES, s));
  TO_HIP(hipMemsetAsync(exch_, 0, used_, s));
}

void XcdExchange::status_reset() {
  status_alloc();
  std::memset(status_, 0, 16);
}

long long watchdog_ticks() {
  static const double timeout_s = [] { const char* e = getenv("TOPS_ONLINE_TIMEOUT_S"); return e ? atof(e) : 2.0; }();
  return (long long)(timeout_s * 100e6);
}

}  // namespace xe

// The exchange needs every participating workgroup on ONE XCD (one L2).  The kernels get that from the dispatcher's
// round-robin -- workgroup b of a grid lands on XCD b % 8 in SPX mode with every CU enabled -- which is observed
// behaviour, not a documented contract: probed once per process with a grid of the same shape (every participating
// workgroup reports the XCC it runs on) before a kernel is ever trusted with parameters.  Other partition modes or a CU
// mask fail the probe and the caller keeps its generic route.
__global__ void online_xcc_probe_kernel(int* out) {
  if (blockIdx.x % 8 != 0 || threadIdx.x != 0) return;
  unsigned xcc;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
  out[blockIdx.x / 8] = (int)(xcc & 0xf);
}

bool xcd_placement_ok(hipStream_t s) {
  static int verdict = -1;
  if (verdict >= 0) return verdict == 1;
  int* host = nullptr;
  if (hipHostMalloc(&host, 32 * sizeof(int), hipHostMallocMapped) != hipSuccess) return false;
  int* dev = nullptr;
  bool ok = hipHostGetDevicePointer(reinterpret_cast<void**>(&dev), host, 0) == hipSuccess;
  for (int rep = 0; ok && rep < 4; ++rep) {   // (four launches: a placement that only sometimes holds is no placement)
    for (int i = 0; i < 32; ++i) host[i] = -1;
    launch_k(online_xcc_probe_kernel, dim3(8 * 32), dim3(64), 0, s, dev);
    ok = hipStreamSynchronize(s) == hipSuccess;
    for (int i = 0; ok && i < 32; ++i) ok = host[i] >= 0 && host[i] == host[0];
  }
  (void)hipHostFree(host);
  verdict = ok ? 1 : 0;
  return ok;
}

}  // namespace to
