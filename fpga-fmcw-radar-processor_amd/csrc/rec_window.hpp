// rec_window.hpp -- what the list-in / list-out objects (plot extractor, beam merger, velocity unfolder)
// share of one lane's work on an ordered record list: the view a lane reads the list through, the split
// of a circular Doppler window into column runs, and the walk over a record's (beam, range, Doppler)
// neighbourhood.  Host and device code (plain C++, no LDS or cross-lane operation in here), so that the
// walk can also be exercised on the CPU.  The tile machinery around it is rec_tiles.hpp.
//
// A record is 16 or 32 bytes (fmcw_det, fmcw_plot, fmcw_mplot, fmcw_vplot) and begins with the words
// frame, range | doppler << 16, mag; the list is ordered by (frame, range, doppler) and holds a cell at
// most once.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/fmcw.h"

#define FMCW_HD __host__ __device__ __forceinline__

namespace fmcw_rec {

FMCW_HD uint32_t umin(uint32_t a, uint32_t b) { return a < b ? a : b; }

FMCW_HD uint64_t make_key(uint32_t f, uint32_t r, uint32_t d) {
  return ((uint64_t)f << 32) | (r << 16) | d;
}

// The list as a lane sees it: records [s_lo, s_lo + s_n) from LDS (s_n = 0: nothing staged), the rest
// from global memory.  n counts the records that take part (those of a frame below the call's n_groups);
// start[m], where there is an index, is the first record of frame m or later, for m = 0 .. n_groups.
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
    const uint32_t rd = p[1];
    return make_key(p[0], rd & 0xffffu, rd >> 16);
  }
  // (range, doppler) as one ascending 32-bit key, read in place: the frame is fixed inside a segment
  FMCW_HD uint32_t cell_key(uint32_t i) const {
    const uint32_t rd = word(i)[1];
    return (rd << 16) | (rd >> 16);
  }
  FMCW_HD float mag(uint32_t i) const {
    const uint32_t j = i - s_lo;
    if (j < s_n) return s_mag[j];
    return reinterpret_cast<const float*>(word(i))[2];
  }
  // frame m's records [lo, hi): the index is trusted only as far as the list reaches
  FMCW_HD void segment(uint32_t m, uint32_t& lo, uint32_t& hi) const {
    hi = umin(start[m + 1], n);
    lo = umin(start[m], hi);
  }
};

// The columns (d - w .. d + w) mod n_doppler as two ascending runs [a(k), b(k)], k = 0, 1; run 1 is
// empty (b1 < a1) unless the window wraps.  o(k) turns a column of run k into its signed offset from d.
// n_doppler >= 2 w + 1, so the runs do not overlap.  Scalars selected by k, not arrays: a lane indexes
// nothing at run time.
struct ColumnRuns {
  int a0, b0, o0, a1, b1, o1;
  FMCW_HD int a(int k) const { return k ? a1 : a0; }
  FMCW_HD int b(int k) const { return k ? b1 : b0; }
  FMCW_HD int o(int k) const { return k ? o1 : o0; }
};
FMCW_HD ColumnRuns column_runs(uint32_t d, uint32_t w, uint32_t n_doppler) {
  const int nd = (int)n_doppler, c_lo = (int)d - (int)w, c_hi = (int)d + (int)w;
  if (c_lo < 0) return {0, c_hi, -(int)d, c_lo + nd, nd - 1, -(int)d - nd};
  if (c_hi >= nd) return {0, c_hi - nd, nd - (int)d, c_lo, nd - 1, -(int)d};
  return {c_lo, c_hi, -(int)d, 0, -1, 0};
}

// A frame is map m = scan * n_beams + beam.  The plot extractor's window is the neighbourhood of a
// geometry with n_beams = 1, win_beam = 0, beam_wrap = 0: every frame is its own scan, only db == 0
// runs and start[] is never read, so that caller's view carries no index.
struct WalkGeom {
  uint32_t n_range, n_doppler, n_beams, win_beam, win_range, win_doppler, beam_wrap;
};

// Calls fn(q, mag(q), db, dr, dd) for every record q of the neighbourhood of P = record i = (map m,
// r, d), P included: maps in ascending db, rows in ascending dr, then the column runs; stops when fn
// returns false.
//
// In a map the searched keys ascend (row by row, run by run), and a cell is listed at most once, so
// after the first search every lower bound lies within n_doppler records of the one before it.  The
// first search of P's own map is bounded by the (win_range + 1) n_doppler records before P, the first
// search of another beam's map by that map's segment [start[m'], start[m' + 1]).  On an unordered
// list the bounds still keep every probe inside [0, n).
template <class F>
FMCW_HD void visit_neighbourhood(const RecView& v, const WalkGeom& g, uint32_t i, uint32_t m, uint32_t r, uint32_t d,
                                 F&& fn) {
  const int wr = (int)g.win_range, wb = (int)g.win_beam, nb = (int)g.n_beams;
  const ColumnRuns c = column_runs(d, g.win_doppler, g.n_doppler);
  const int runs = c.b1 < c.a1 ? 1 : 2;
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
      v.segment(mm, lo, hi);
      if (lo == hi) continue;   // no record of that beam
    }
    for (int dr = -wr; dr <= wr; ++dr) {
      const int rr = (int)r + dr;
      if (rr < 0 || rr >= (int)g.n_range) continue;
      for (int k = 0; k < runs; ++k) {
        const uint64_t ka = make_key(mm, (uint32_t)rr, (uint32_t)c.a(k)), kb = make_key(mm, (uint32_t)rr, (uint32_t)c.b(k));
        while (lo < hi) {
          const uint32_t mid = (lo + hi) >> 1;
          if (v.key(mid) < ka) lo = mid + 1;
          else hi = mid;
        }
        uint32_t q = lo;
        for (int left = c.b(k) - c.a(k); left >= 0 && q < v.n; --left, ++q) {
          const uint64_t kq = v.key(q);
          if (kq > kb) break;
          if (!fn(q, v.mag(q), db, dr, (int)(kq & 0xffffu) + c.o(k))) return;
        }
        hi = umin(v.n, lo + g.n_doppler);
      }
    }
  }
}

}  // namespace fmcw_rec
