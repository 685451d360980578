// spec_rows.hpp -- mti_point: the MTI canceller over a [chirp] row of fmcw_range_ct's plain spectrum.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/fmcw.h"

namespace fmcw {

// The canceller of k_beams, k_adapt_acc and k_bearings, stated once: y[c] = x[c] - x[c-1] (2-pulse) or
// x[c] - 2 x[c-1] + x[c-2] (3-pulse; left to right, per component), with a zero delay line before
// chirp 0 whatever lies before the row in memory.  p points at x[c] of a row, c is its chirp.  The
// predecessors are loaded from a clamped address (p[0] where the row has none) and dropped afterwards:
// nothing outside the row is read and no branch surrounds a load, so a caller's loads of several
// channels stay in flight together.
// K2 (doppler_kernel.hpp) restates the rule and is no caller: it reads through at() over the three
// spectrum forms, carries the integer RTL-compatible datapath as well, and is the measured path.
template <int MTI>
__device__ __forceinline__ float2 mti_point(const float2* __restrict__ p, uint32_t c) {
  float2 x = p[0];
  if constexpr (MTI != FMCW_MTI_OFF) {
    const int b1 = c >= 1 ? 1 : 0;
    float2 x1 = p[-b1];
    x1 = b1 ? x1 : make_float2(0.f, 0.f);
    if constexpr (MTI == FMCW_MTI_2PULSE) {
      x.x -= x1.x;
      x.y -= x1.y;
    } else {
      const int b2 = c >= 2 ? 2 : 0;
      float2 x2 = p[-b2];
      x2 = b2 ? x2 : make_float2(0.f, 0.f);
      x.x = x.x - 2.f * x1.x + x2.x;
      x.y = x.y - 2.f * x1.y + x2.y;
    }
  }
  return x;
}

}  // namespace fmcw
