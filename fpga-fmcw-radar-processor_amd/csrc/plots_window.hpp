// plots_window.hpp -- the window walk of the plot extractor (fmcw_plots.hip): the list view a lane
// searches and the visit of one detection's window.  Host and device code (plain C++, no LDS or
// cross-lane operation in here), so that the walk can also be exercised on the CPU.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/fmcw.h"

#define FMCW_HD __host__ __device__ __forceinline__

namespace fmcw_plots {

FMCW_HD uint32_t umin(uint32_t a, uint32_t b) { return a < b ? a : b; }

struct PlotGeom {
  uint32_t n_range, n_doppler, win_range, win_doppler;
};

FMCW_HD uint64_t make_key(uint32_t f, uint32_t r, uint32_t d) {
  return ((uint64_t)f << 32) | (r << 16) | d;
}

// The list as a lane sees it: records [s_lo, s_lo + s_n) from LDS, the rest from global memory.
struct ListView {
  const fmcw_det* dets;
  uint32_t n, s_lo, s_n;
  const uint64_t* s_key;
  const float* s_mag;
  FMCW_HD uint64_t key(uint32_t i) const {
    const uint32_t j = i - s_lo;
    if (j < s_n) return s_key[j];
    return make_key(dets[i].frame, dets[i].range, dets[i].doppler);
  }
  FMCW_HD float mag(uint32_t i) const {
    const uint32_t j = i - s_lo;
    return j < s_n ? s_mag[j] : dets[i].mag;
  }
};

// Calls fn(q, mag(q), dr, dd) for every detection q of the window of P = record i = (f, r, d), P
// included, rows in ascending dr; stops when fn returns false.
template <class F>
FMCW_HD void visit_window(const ListView& v, const PlotGeom& g, uint32_t i, uint32_t f, uint32_t r, uint32_t d,
                          F&& fn) {
  const int nd = (int)g.n_doppler, wd = (int)g.win_doppler, wr = (int)g.win_range;
  const int c_lo = (int)d - wd, c_hi = (int)d + wd;
  // column runs [a, b] with the offset that turns a column into dd
  int ra[2], rb[2], ro[2], runs = 1;
  if (c_lo < 0) {
    ra[0] = 0, rb[0] = c_hi, ro[0] = -(int)d;
    ra[1] = c_lo + nd, rb[1] = nd - 1, ro[1] = -(int)d - nd;
    runs = 2;
  } else if (c_hi >= nd) {
    ra[0] = 0, rb[0] = c_hi - nd, ro[0] = nd - (int)d;
    ra[1] = c_lo, rb[1] = nd - 1, ro[1] = -(int)d;
    runs = 2;
  } else {
    ra[0] = c_lo, rb[0] = c_hi, ro[0] = -(int)d;
  }
  for (int dr = -wr; dr <= wr; ++dr) {
    const int rr = (int)r + dr;
    if (rr < 0 || rr >= (int)g.n_range) continue;
    // a cell is listed at most once, so row rr of frame f lies within `span` records of P
    const uint32_t span = (uint32_t)((dr < 0 ? -dr : dr) + 1) * g.n_doppler;
    const uint32_t lo0 = i - umin(i, span), hi0 = umin(v.n, i + 1 + span);
    for (int k = 0; k < runs; ++k) {
      const uint64_t ka = make_key(f, (uint32_t)rr, (uint32_t)ra[k]), kb = make_key(f, (uint32_t)rr, (uint32_t)rb[k]);
      uint32_t lo = lo0, hi = hi0;
      while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (v.key(mid) < ka) lo = mid + 1;
        else hi = mid;
      }
      for (int c = rb[k] - ra[k]; c >= 0 && lo < v.n; --c, ++lo) {
        const uint64_t kq = v.key(lo);
        if (kq > kb) break;
        if (!fn(lo, v.mag(lo), dr, (int)(kq & 0xffffu) + ro[k])) return;
      }
    }
  }
}

}  // namespace fmcw_plots
