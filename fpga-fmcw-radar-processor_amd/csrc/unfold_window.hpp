// unfold_window.hpp -- what one lane of the velocity unfolder (fmcw_unfold.hip) does for one record of
// one dwell: the (dwell, stream, position) numbering, the hit search in another scan's segment and the
// walk over the hypotheses, over the list view and the column runs of rec_window.hpp (nothing staged:
// the view reads in place).  Host and device code (plain C++, no LDS or cross-lane operation), so that
// it can also be exercised on the CPU.
//
// Integers: see include/fmcw.h -- |v| <= v_max < 2^31 and |v / p| <= 32 n_doppler + 1, so int32 holds
// every intermediate; floor((2 v + p) / (2 p)) is floor(v / p) plus one if twice the remainder reaches p.
#pragma once
#include "rec_window.hpp"

namespace fmcw_unfold {

using fmcw_rec::RecView;
using fmcw_rec::umin;

constexpr uint32_t kNone = 0xffffffffu;

struct UnfoldGeom {
  uint32_t n_range, n_doppler, n_prf, prf_phase, step, zero_bin, v_max, out_unit, tol_range, tol_doppler, m_of,
      n_streams;
  uint64_t units_lo, units_hi;   // prf_units[0..3], [4..7], 16 bits each: selected by shifts, not by an index
};

FMCW_HD uint32_t prf_unit(const UnfoldGeom& g, uint32_t k) {
  const uint64_t w = k < 4 ? g.units_lo : g.units_hi;
  return (uint32_t)(w >> (16 * (k & 3))) & 0xffffu;
}
// the PRF unit of scan s
FMCW_HD uint32_t scan_unit(const UnfoldGeom& g, uint32_t s) { return prf_unit(g, (s + g.prf_phase) % g.n_prf); }

FMCW_HD int floordiv(int a, int b) {   // b > 0
  int q = a / b;
  if (a - q * b < 0) --q;
  return q;
}

// One (dwell, stream, position) triple q = (j n_streams + t) K + i and its frame m = (j step + i) n_streams + t.
struct Slot {
  uint32_t j, t, i, m;
};
FMCW_HD Slot slot_of(const UnfoldGeom& g, uint32_t q) {
  Slot s;
  s.i = q % g.n_prf;
  const uint32_t jt = q / g.n_prf;
  s.t = jt % g.n_streams;
  s.j = jt / g.n_streams;
  s.m = (s.j * g.step + s.i) * g.n_streams + s.t;
  return s;
}

// The record of largest mag among (r + dr, (d + dd) mod n_doppler), |dr| <= tol_range, |dd| <= tol_doppler, in
// the segment [lo, hi) of one frame; the first in list order among equals; kNone if there is none.
// Rows ascend and the (at most two) column runs of a row ascend, so the records are met in list
// order and every lower bound lies at or after the one before it.
FMCW_HD uint32_t window_hit(const RecView& l, const UnfoldGeom& g, uint32_t lo, const uint32_t hi, uint32_t r, uint32_t d) {
  if (lo >= hi) return kNone;
  const int tr = (int)g.tol_range;
  const fmcw_rec::ColumnRuns c = fmcw_rec::column_runs(d, g.tol_doppler, g.n_doppler);
  uint32_t best = kNone;
  float best_mag = 0.f;
  for (int dr = -tr; dr <= tr; ++dr) {
    const int rr = (int)r + dr;
    if (rr < 0 || rr >= (int)g.n_range) continue;
    for (int run = 0; run < 2; ++run) {
      const int a = c.a(run), b = c.b(run);
      if (b < a) continue;
      const uint32_t ka = ((uint32_t)rr << 16) | (uint32_t)a, kb = ((uint32_t)rr << 16) | (uint32_t)b;
      uint32_t top = hi;
      while (lo < top) {
        const uint32_t mid = (lo + top) >> 1;
        if (l.cell_key(mid) < ka) lo = mid + 1;
        else top = mid;
      }
      for (; lo < hi; ++lo) {
        if (l.cell_key(lo) > kb) break;
        const float mq = l.mag(lo);
        if (best == kNone || mq > best_mag) best = lo, best_mag = mq;
      }
    }
  }
  return best;
}

// The signed bin of d and the range of m with |(ds + m n_doppler) p| <= v_max (empty if m_lo > m_hi).
FMCW_HD void hypothesis_range(const UnfoldGeom& g, uint32_t d, uint32_t p, int& ds, int& m_lo, int& m_hi) {
  const int nd = (int)g.n_doppler;
  ds = (int)d - (int)g.zero_bin;
  if (ds < 0) ds += nd;
  if (ds >= (nd + 1) / 2) ds -= nd;
  const int lim = (int)(g.v_max / p);   // <= 32 n_doppler
  m_lo = -floordiv(lim + ds, nd);
  m_hi = floordiv(lim - ds, nd);
}

// the bin v folds to at a PRF of p units
FMCW_HD uint32_t predicted_bin(const UnfoldGeom& g, int v, uint32_t p) {
  int q = v / (int)p, rem = v - q * (int)p;
  if (rem < 0) --q, rem += (int)p;
  if (2 * rem >= (int)p) ++q;
  int x = q % (int)g.n_doppler;
  if (x < 0) x += (int)g.n_doppler;
  x += (int)g.zero_bin;
  if (x >= (int)g.n_doppler) x -= (int)g.n_doppler;
  return (uint32_t)x;
}

// Calls fn(position, record) for every hit of hypothesis v of record idx = (slot s, range r), in
// ascending position; the record's own position is a hit with the record itself.
template <class F>
FMCW_HD void visit_hits(const RecView& l, const UnfoldGeom& g, const Slot& s, uint32_t idx, uint32_t r, int v, F&& fn) {
  for (uint32_t i2 = 0; i2 < g.n_prf; ++i2) {
    if (i2 == s.i) {
      fn(i2, idx);
      continue;
    }
    const uint32_t s2 = s.j * g.step + i2;
    uint32_t lo, hi;
    l.segment(s2 * g.n_streams + s.t, lo, hi);
    if (lo == hi) continue;
    const uint32_t q = window_hit(l, g, lo, hi, r, predicted_bin(g, v, scan_unit(g, s2)));
    if (q != kNone) fn(i2, q);
  }
}

struct Verdict {
  bool report;
  int fold;          // m of the best hypothesis
  uint32_t n_ties;   // hypotheses with its hit count
};

// Every hypothesis of record idx = (slot s, r, d): the best one, and whether the record reports.
FMCW_HD Verdict judge(const RecView& l, const UnfoldGeom& g, const Slot& s, uint32_t idx, uint32_t r, uint32_t d) {
  const uint32_t p = scan_unit(g, s.j * g.step + s.i);
  int ds, m_lo, m_hi;
  hypothesis_range(g, d, p, ds, m_lo, m_hi);
  uint32_t best_hits = 0, best_mask = 0, best_abs = 0, ties = 0;
  int best_m = 0;
  for (int m = m_lo; m <= m_hi; ++m) {
    const int v = (ds + m * (int)g.n_doppler) * (int)p;
    uint32_t mask = 0;
    visit_hits(l, g, s, idx, r, v, [&](uint32_t i2, uint32_t) { mask |= 1u << i2; });
    const uint32_t hits = (uint32_t)__builtin_popcount(mask), av = (uint32_t)(v < 0 ? -v : v);
    if (hits > best_hits) ties = 1;
    else if (hits == best_hits) ++ties;
    if (hits > best_hits || (hits == best_hits && av < best_abs)) best_hits = hits, best_mask = mask, best_abs = av, best_m = m;
  }
  Verdict out;
  // no hypothesis at all leaves best_hits 0 < m_of
  out.report = best_hits >= g.m_of && !(best_mask & ((1u << s.i) - 1u));
  out.fold = best_m;
  out.n_ties = umin(ties, 65535u);
  return out;
}

// The report of record idx for its best hypothesis (fold, n_ties from judge()).
FMCW_HD fmcw_vplot report(const RecView& l, const UnfoldGeom& g, const Slot& s, uint32_t idx, int fold, uint32_t n_ties) {
  const uint32_t rd = l.word(idx)[1], r = rd & 0xffffu, d = rd >> 16;
  const uint32_t p = scan_unit(g, s.j * g.step + s.i);
  int ds, m_lo, m_hi;
  hypothesis_range(g, d, p, ds, m_lo, m_hi);
  const int v = (ds + fold * (int)g.n_doppler) * (int)p;
  uint32_t mask = 0;
  float sum = 0.f;
  visit_hits(l, g, s, idx, r, v, [&](uint32_t i2, uint32_t q) {
    mask |= 1u << i2;
    sum += l.mag(q);
  });
  const uint32_t a = (uint32_t)v + g.v_max;   // v + v_max in 0 .. 2 v_max
  const uint32_t q = a / g.out_unit, rem = a - q * g.out_unit;
  fmcw_vplot o;
  o.frame = s.j * g.n_streams + s.t;
  o.range = (uint16_t)r;
  o.doppler = (uint16_t)(q + (2 * rem >= g.out_unit ? 1u : 0u));
  o.mag = l.mag(idx);
  o.v_fine = v;
  o.fold = (int16_t)fold;
  o.n_hits = (uint8_t)__builtin_popcount(mask);
  o.hit_mask = (uint8_t)mask;
  o.sum_mag = sum;
  o.pos = (uint16_t)s.i;
  o.n_ties = (uint16_t)n_ties;
  o.src = idx;
  return o;
}

}  // namespace fmcw_unfold
