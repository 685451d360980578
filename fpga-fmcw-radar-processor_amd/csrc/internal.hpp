// internal.hpp -- error plumbing shared by the host translation units of libfmcw.so.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "../../include/fmcw.h"

namespace fmcw {

// Sets the calling thread's fmcw_last_error() message (printf format; the one thread-local
// string lives in fmcw_api.hip) and returns `code`.
int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
// FMCW_OK, or FMCW_EHIP with the pending launch error of kernel `what`
int check_launch(const char* what);
// The fp32 window table of n points the kernels multiply by (fmcw_api.hip): FMCW_WIN_HAMMING, or
// ones for FMCW_WIN_NONE, scaled by 2^-shift; FMCW_WIN_Q15_RTL gives the ROM integers.
std::vector<float> window_table(uint32_t n, int kind, uint32_t shift = 0);

}  // namespace fmcw

#define HIP_TRY(expr)                                                                          \
  do {                                                                                         \
    hipError_t e_ = (expr);                                                                    \
    if (e_ != hipSuccess) return fmcw::fail(FMCW_EHIP, "%s: %s (%s:%d)", #expr,                \
                                            hipGetErrorString(e_), __FILE__, __LINE__);        \
  } while (0)
