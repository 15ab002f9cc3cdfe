// common.h — error plumbing for the C ABI (thread-local last-error message; no C++
// exception crosses the ABI boundary).
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>

#include "../../include/az_othello.h"

namespace azc {

int set_error(int code, const char* fmt, ...);

inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

}  // namespace azc

#define AZ_HIP(call)                                                                  \
  do {                                                                                \
    hipError_t e_ = (call);                                                           \
    if (e_ != hipSuccess)                                                             \
      return azc::set_error(AZ_ERR_HIP, "%s failed: %s (%s:%d)", #call,               \
                            hipGetErrorString(e_), __FILE__, __LINE__);               \
  } while (0)

#define AZ_REQUIRE(cond, code, ...)                                                   \
  do {                                                                                \
    if (!(cond)) return azc::set_error((code), __VA_ARGS__);                          \
  } while (0)

// The FP16X2 kernels' scale exponent, from the bits of a max |x| word (a non-negative finite
// float): frexp's e (max < 2^e), never below AZ_SCALE_EXP_MIN; 0 -> 0.  Operands are scaled by
// 2^(15 - e) (13 - e for Winograd's transformed inputs) before the fp16 hi / lo split, and the
// epilogue removes 2^(scale of the inputs + scale of the weights).  Unclamped, a max below
// 2^-112 asked for 2^128 = inf (every zero of the board then 0 * inf = NaN).  With the clamp no
// scale exceeds 2^115, and a removal factor whose exponent (two scales added, as low as -230)
// falls below fp32's range underflows to 0 where the product itself does.  Maxima below
// 2^-101 keep fewer bits (the scaled values sink into fp16's subnormals and vanish below
// 2^-139): an absolute error of at most 2^-140 per input value.
// Every site takes the scale and its removal from this one function, so the removal is exact.
#define AZ_SCALE_EXP_MIN (-100)
__device__ __forceinline__ int az_scale_exp(unsigned max_bits) {
  const int e = (int)((max_bits >> 23) & 0xff) - 126;
  return max_bits == 0u ? 0 : (e < AZ_SCALE_EXP_MIN ? AZ_SCALE_EXP_MIN : e);
}

// Wrap an entry point body so no C++ exception (e.g. std::bad_alloc) escapes.
#define AZ_GUARD_BEGIN try {
#define AZ_GUARD_END                                                                  \
  }                                                                                   \
  catch (const std::exception& ex) {                                                  \
    return azc::set_error(AZ_ERR_ARG, "exception: %s", ex.what());                    \
  }                                                                                   \
  catch (...) {                                                                       \
    return azc::set_error(AZ_ERR_ARG, "unknown exception");                           \
  }
