// merge_window.hpp -- the neighbourhood walk of the beam merger (fmcw_merge.hip): the list view a
// lane searches and the visit of one record's (beam, range, Doppler) neighbourhood.  Host and device
// code (plain C++, no LDS or cross-lane operation in here), so that the walk can also be exercised on
// the CPU.
//
// plots_window.hpp's visit_window is bound to its ListView, which indexes an fmcw_det array (stride
// 16) and searches one map.  The merger reads records of stride 16 or 32 and searches up to nine
// maps, so the walk is restated here over a view that carries the stride and the map index; the key
// packing, the column runs and the bounded lower-bound search are those of the plot extractor.
#pragma once
#include "plots_window.hpp"

namespace fmcw_merge {

using fmcw_plots::make_key;
using fmcw_plots::umin;

struct MergeGeom {
  uint32_t n_range, n_doppler, n_beams, win_beam, win_range, win_doppler, beam_wrap;
};

// The list as a lane sees it: records [s_lo, s_lo + s_n) from LDS, the rest from global memory.
// n counts the records that take part (those of a map below n_maps); start[m] is the first record
// of map m or later, for m = 0 .. n_maps.
struct RecView {
  const uint8_t* recs;
  uint32_t stride, n, s_lo, s_n;
  const uint64_t* s_key;
  const float* s_mag;
  const uint32_t* start;
  FMCW_HD const uint32_t* word(uint32_t i) const {
    return reinterpret_cast<const uint32_t*>(recs + (size_t)i * stride);
  }
  FMCW_HD uint64_t key(uint32_t i) const {
    const uint32_t j = i - s_lo;
    if (j < s_n) return s_key[j];
    const uint32_t* p = word(i);
    const uint32_t rd = p[1];   // range | doppler << 16
    return make_key(p[0], rd & 0xffffu, rd >> 16);
  }
  FMCW_HD float mag(uint32_t i) const {
    const uint32_t j = i - s_lo;
    if (j < s_n) return s_mag[j];
    return reinterpret_cast<const float*>(word(i))[2];
  }
};

// Calls fn(q, mag(q), db, dr, dd) for every record q of the neighbourhood of P = record i = (map m,
// r, d), P included: maps in ascending db, rows in ascending dr, then the column runs; stops when fn
// returns false.
//
// In a map the searched keys ascend (row by row, run by run), and a cell is listed at most once, so
// after the first search every lower bound lies within n_doppler records of the one before it.  The
// first search of P's own map is bounded by the (win_range + 1) n_doppler records before P, the first
// search of another beam's map by that map's segment [start[m'], start[m' + 1]).
template <class F>
FMCW_HD void visit_neighbourhood(const RecView& v, const MergeGeom& g, uint32_t i, uint32_t m, uint32_t r, uint32_t d,
                                 F&& fn) {
  const int nd = (int)g.n_doppler, wd = (int)g.win_doppler, wr = (int)g.win_range, wb = (int)g.win_beam;
  const int nb = (int)g.n_beams;
  const int c_lo = (int)d - wd, c_hi = (int)d + wd;
  // column runs [a, b], ascending, with the offset that turns a column into dd
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
  const int b = (int)(m % g.n_beams);
  const uint32_t m0 = m - (uint32_t)b;   // the scan's first map
  for (int db = -wb; db <= wb; ++db) {
    int bb = b + db;
    if (bb < 0 || bb >= nb) {
      if (!g.beam_wrap) continue;
      bb += bb < 0 ? nb : -nb;   // n_beams >= 2 win_beam + 1: one turn at most, and no beam twice
    }
    const uint32_t mm = m0 + (uint32_t)bb;
    uint32_t lo, hi;   // the next lower bound lies in [lo, hi]
    if (db == 0) {
      lo = i - umin(i, (uint32_t)(wr + 1) * g.n_doppler);
      hi = i;          // the first key searched is not above P's
    } else {
      hi = umin(v.start[mm + 1], v.n);   // the index is trusted only as far as the list reaches
      lo = umin(v.start[mm], hi);
      if (lo == hi) continue;            // no record of that beam
    }
    for (int dr = -wr; dr <= wr; ++dr) {
      const int rr = (int)r + dr;
      if (rr < 0 || rr >= (int)g.n_range) continue;
      for (int k = 0; k < runs; ++k) {
        const uint64_t ka = make_key(mm, (uint32_t)rr, (uint32_t)ra[k]), kb = make_key(mm, (uint32_t)rr, (uint32_t)rb[k]);
        while (lo < hi) {
          const uint32_t mid = (lo + hi) >> 1;
          if (v.key(mid) < ka) lo = mid + 1;
          else hi = mid;
        }
        uint32_t q = lo;
        for (int c = rb[k] - ra[k]; c >= 0 && q < v.n; --c, ++q) {
          const uint64_t kq = v.key(q);
          if (kq > kb) break;
          if (!fn(q, v.mag(q), db, dr, (int)(kq & 0xffffu) + ro[k])) return;
        }
        hi = umin(v.n, lo + g.n_doppler);
      }
    }
  }
}

}  // namespace fmcw_merge
