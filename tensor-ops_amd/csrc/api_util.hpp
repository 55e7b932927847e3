// What a file of extern "C" entry points (api.cpp, stack_ff.cpp, stack_rnn.cpp) wraps every entry in: the library lock, the
// entry clock, the calling thread's device, and the translation of exceptions into a status + to_last_error().
#pragma once
#include <chrono>

#include "ops.hpp"

namespace to {
extern thread_local std::string g_err;  // to_last_error (api.cpp)
}

// HIP's current device is per OS thread and to_init selects it on the initialising thread only: a Haskell
// capability (or any second thread) calling in would otherwise allocate and load modules on device 0.
inline void bind_device() {
  static thread_local int bound = -1;
  to::Runtime& r = to::rt();
  if (r.inited && bound != r.device) {
    (void)hipSetDevice(r.device);
    bound = r.device;
  }
}

// host time spent inside the library's entry points (to_api_time): what a host's own per-step cost is NOT
// (the time-stamp counter, not clock_gettime: two calls of the latter per entry point were 2 us of a 40 us step)
// (x86-64: an invariant TSC, synchronised across cores, is assumed -- every x86 server part of the last decade; elsewhere the
//  compiler's cycle counter where it has one (aarch64: cntvct), else the steady clock.  Calibrated once against steady_clock.)
#if defined(__x86_64__) || defined(__i386__)
static inline uint64_t api_ticks() { return __builtin_ia32_rdtsc(); }
#elif defined(__aarch64__)
static inline uint64_t api_ticks() {
  uint64_t v;
  asm volatile("mrs %0, cntvct_el0" : "=r"(v));
  return v;
}
#else
static inline uint64_t api_ticks() {
  return (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
#endif
struct ApiClock {
  const char* fn;
  uint64_t t0 = api_ticks();
  explicit ApiClock(const char* f) : fn(f) {}
  ~ApiClock();  // api.cpp, beside the counters it adds to
};

#define API_BEGIN                                          \
  std::lock_guard<std::recursive_mutex> guard_(to::lock()); \
  ApiClock clock_(__func__);                                \
  bind_device();                                            \
  try {
#define API_END                          \
  return TO_OK;                          \
  }                                      \
  catch (const to::Error& e) {           \
    to::g_err = e.what();                \
    return e.code;                       \
  }                                      \
  catch (const std::exception& e) {      \
    to::g_err = e.what();                \
    return TO_ERR_ARG;                   \
  }
// like API_END but falls through on success
#define API_END_CHECK                    \
  }                                      \
  catch (const to::Error& e) {           \
    to::g_err = e.what();                \
    return e.code;                       \
  }
#define NONNULL(p) TO_CHECK((p) != nullptr, TO_ERR_ARG, "null argument: " #p)
