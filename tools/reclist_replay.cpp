// reclist_replay.cpp -- the record-list layer of the plot extractor, the beam merger and the velocity
// unfolder (csrc/rec_window.hpp, csrc/unfold_window.hpp, PeakSums of csrc/rec_tiles.hpp) run on the CPU:
// one call's launches replayed one after another, serially, over heap buffers of exactly the size the
// shipped code is entitled to, so that under AddressSanitizer a probe one element out of bounds is a
// report and not a fault on a GPU.  Built host-only with ASan and UBSan by tools/reclist_replay.sh and
// driven by tests/test_reclist_replay.py.
//
//   reclist_replay CASE RESULT        exit 0: RESULT written; 2: CASE refused; 3: a check of the replay failed
//
// From the shipped headers: make_key, RecView (key, mag, cell_key, word, segment), column_runs,
// visit_neighbourhood, PeakSums::centre, slot_of, window_hit, hypothesis_range, predicted_bin, visit_hits,
// judge, report.  Restated here, because they are device code (ballots, LDS, the tile scan, lambdas in
// kernels): the per-item rule of k_frame_index, stage_tile, the bodies of find_peaks / emit_peaks around
// the walk, scan_status, k_unfold_dwells, locate, the bodies of k_unfold_find / _scan / _emit around
// judge() and report(), the three record writers, the create / enqueue argument checks and plan_list.
// A ballot mask is a bit per item (item j of tile t: bit j % 64 of masks[t * groups + j / 64], which
// is where the kernels' group numbering puts it), a scan is a prefix sum.
//
// The tiles are the shipped ones: 1024 records with a 512-record halo (plots, merge), 1024 pairs
// (unfold).  The find and emit passes of plots and merge read through a RecView whose staged span
// [s_lo, s_lo + s_n) is copied into arrays of their own of exactly s_n entries, as stage_tile does.
//
// CASE (little-endian 32-bit words): a header of 40 words, then rec_bytes bytes of records.
//    0  magic 0x50524c52 ("RLRP")
//    1  object: 0 plots, 1 merge, 2 unfold
//    2  rec_stride (16 or 32; plots: 16)
//    3  rec_cap
//    4  max_recs (max_dets)
//    5  the n_recs word
//    6  n_maps (merge), n_scans (unfold), 0 (plots)
//    7  out_cap
//    8  rec_bytes: the first min(rec_cap, max_recs) * rec_stride of them are what the call may read; a
//       shorter list is padded with 0xA5 bytes
//    9  max_maps / max_frames (0 for plots)
//   10..  configuration
//         plots:  n_range, n_doppler, win_range, win_doppler
//         merge:  n_range, n_doppler, n_beams, win_beam, win_range, win_doppler, beam_wrap
//         unfold: n_range, n_doppler, n_prf, prf_units[8], prf_phase, step, zero_bin, v_max, out_unit,
//                 tol_range, tol_doppler, m_of, n_streams
//   39  0, or k: after the frame index is built, every k-th word of start[] is overwritten with a value far
//       above the list's length, which no call produces; RecView::segment promises to trust the index only
//       as far as the list reaches, and the words of a freshly built index never test that
// RESULT: 8 words, then out_cap 32-byte output slots (filled with 0xA5 before the call).
//    0  magic 0x53524c52 ("RLRS")
//    1  number of status words (plots 2, merge 3, unfold 4)
//    2..5  the status words (0xA5A5A5A5 where the object has none)
//    6  set bits in the masks of the call's tiles
//    7  out_cap
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rec_tiles.hpp"
#include "unfold_window.hpp"

namespace {

using namespace fmcw_rec;
using fmcw_unfold::Slot;
using fmcw_unfold::UnfoldGeom;

constexpr uint32_t kTile = 1024, kGroups = kTile / 64, kHalo = 512;
constexpr uint32_t kFill = 0xA5A5A5A5u;

[[noreturn]] void die(int code, const char* what) {
  fprintf(stderr, "reclist_replay: %s\n", what);
  exit(code);
}
#define REFUSE(cond) do { if (cond) die(2, "case refused: " #cond); } while (0)

// n elements, no byte more, filled with 0xA5
template <class T>
T* exact(size_t n) {
  T* p = static_cast<T*>(malloc(n * sizeof(T)));
  if (!p) die(3, "out of memory");
  memset(static_cast<void*>(p), 0xA5, n * sizeof(T));
  return p;
}

struct Case {
  uint32_t object, stride, rec_cap, max_recs, n_word, n_arg, out_cap, rec_bytes, max_groups, cfg[30];
  const uint8_t* bytes;   // rec_bytes of them
};

// internal.hpp plan_list, without the grids
struct Plan {
  uint32_t cap, tiles;
};
Plan plan_list(const Case& c, uint32_t items_per_rec) {
  Plan p;
  p.cap = umin(c.rec_cap, c.max_recs);
  p.tiles = (uint32_t)(((uint64_t)p.cap * items_per_rec + kTile - 1) / kTile);
  return p;
}

// What the launches of one call share (RecList of rec_tiles.hpp)
struct List {
  const uint8_t* recs;
  uint32_t stride, cap, n_word;
  uint32_t* start;   // n_groups + 1 words, or null
  uint32_t n_groups;
  uint32_t examined() const { return umin(n_word, cap); }
  uint32_t frame(uint32_t i) const { return *reinterpret_cast<const uint32_t*>(recs + (size_t)i * stride); }
};

// k_frame_index, SkipEmpty
void frame_index(const List& l) {
  const uint32_t n = l.examined();
  if (!n) return;
  const int64_t G = (int64_t)l.n_groups;
  for (uint32_t i = 0; i <= n; ++i) {
    const int64_t prev = i ? (int64_t)l.frame(i - 1) : -1;
    int64_t cur = G;
    if (i < n) cur = std::min((int64_t)l.frame(i), G);
    for (int64_t m = prev + 1; m <= cur; ++m) l.start[m] = i;
  }
}

// case word 39
void damage_index(const List& l, uint32_t k) {
  if (!k || !l.start || !l.examined()) return;
  for (uint32_t m = k - 1; m <= l.n_groups; m += k) l.start[m] = 0xffffffffu - m;
}

void set_bit(uint64_t* masks, uint32_t t, uint32_t j) { masks[(size_t)t * kGroups + j / 64] |= 1ull << (j % 64); }
// Tiles::rank: whether item j of tile t is kept, and off + the kept items before it in the tile
bool rank_of(const uint64_t* masks, uint32_t t, uint32_t j, uint32_t off, uint32_t& rank) {
  const uint64_t* m = masks + (size_t)t * kGroups;
  rank = off;
  for (uint32_t g = 0; g < j / 64; ++g) rank += (uint32_t)__builtin_popcountll(m[g]);
  rank += (uint32_t)__builtin_popcountll(m[j / 64] & ((1ull << (j % 64)) - 1ull));
  return (m[j / 64] >> (j % 64)) & 1ull;
}
// tile_offsets_scan: cnt -> its exclusive scan in place; the sum
uint32_t scan(uint32_t* cnt, uint32_t n) {
  uint32_t sum = 0;
  for (uint32_t t = 0; t < n; ++t) {
    const uint32_t c = cnt[t];
    cnt[t] = sum;
    sum += c;
  }
  return sum;
}
uint32_t set_bits(const uint64_t* masks, uint32_t n_tiles) {
  uint32_t c = 0;
  for (size_t g = 0; g < (size_t)n_tiles * kGroups; ++g) c += (uint32_t)__builtin_popcountll(masks[g]);
  return c;
}

struct Out {
  uint8_t* slots;   // out_cap x 32 bytes
  uint32_t cap;
  template <class R>
  void put(uint32_t rank, const R& r) {
    static_assert(sizeof(R) == 32, "output records are 32 bytes");
    if (rank >= cap) die(3, "a rank at or above out_cap reached the record writer");
    memcpy(slots + (size_t)rank * 32, &r, 32);
  }
};

// ---- plots and merge -----------------------------------------------------------------------------

// rec_tiles.hpp in_use()
uint32_t in_use(const List& l) {
  const uint32_t n = l.examined();
  return n && l.start ? umin(l.start[l.n_groups], n) : n;
}

// stage_tile: the staged span in arrays of exactly s_n entries
struct Staged {
  RecView v;
  uint64_t* key;
  float* mag;
  Staged(const List& l, uint32_t n, uint32_t base) {
    v.recs = l.recs;
    v.stride = l.stride;
    v.n = n;
    v.s_lo = base > kHalo ? base - kHalo : 0u;
    v.s_n = umin(n, base + kTile + kHalo) - v.s_lo;
    key = exact<uint64_t>(v.s_n);
    mag = exact<float>(v.s_n);
    v.s_key = key;
    v.s_mag = mag;
    v.start = l.start;
    for (uint32_t j = 0; j < v.s_n; ++j) {
      const uint32_t* p = v.word(v.s_lo + j);
      const uint32_t rd = p[1];
      key[j] = make_key(p[0], rd & 0xffffu, rd >> 16);
      memcpy(&mag[j], &p[2], 4);
    }
  }
  ~Staged() {
    free(key);
    free(mag);
  }
};

void find_peaks(const List& l, const WalkGeom& g, uint64_t* masks, uint32_t* tile_cnt) {
  const uint32_t n = in_use(l), n_tiles = (n + kTile - 1) / kTile;
  for (uint32_t t = 0; t < n_tiles; ++t) {
    const uint32_t base = t * kTile;
    const Staged st(l, n, base);
    const RecView& v = st.v;
    for (uint32_t g2 = 0; g2 < kGroups; ++g2) masks[(size_t)t * kGroups + g2] = 0;
    uint32_t cnt = 0;
    for (uint32_t j = 0; j < kTile; ++j) {
      const uint32_t i = base + j;
      bool peak = false;
      if (i < n) {
        const uint64_t kp = v.key(i);
        const float mp = v.mag(i);
        peak = !l.start || (uint32_t)(kp >> 32) < l.n_groups;
        if (peak)
          visit_neighbourhood(v, g, i, (uint32_t)(kp >> 32), (uint32_t)(kp >> 16) & 0xffffu, (uint32_t)kp & 0xffffu,
                              [&](uint32_t q, float mq, int, int, int) {
                                if (q != i && (mq > mp || (mq == mp && q < i))) peak = false;
                                return peak;
                              });
      }
      if (peak) set_bit(masks, t, j), ++cnt;
    }
    tile_cnt[t] = cnt;
  }
}

void scan_status(const List& l, uint32_t* tile_cnt, uint32_t* status) {
  const uint32_t found = l.n_word, n = umin(found, l.cap), use = in_use(l);
  status[0] = scan(tile_cnt, (use + kTile - 1) / kTile);
  status[1] = found - n;
  if (l.start) status[2] = n - use;
}

template <class W>
void emit_peaks(const List& l, const WalkGeom& g, const uint64_t* masks, const uint32_t* tile_off, uint32_t out_cap,
                W&& write) {
  const uint32_t n = in_use(l), n_tiles = (n + kTile - 1) / kTile;
  for (uint32_t t = 0; t < n_tiles; ++t) {
    const uint32_t base = t * kTile, off = tile_off[t];
    if (off >= out_cap) break;
    const Staged st(l, n, base);
    const RecView& v = st.v;
    for (uint32_t j = 0; j < kTile; ++j) {
      uint32_t rank;
      if (!rank_of(masks, t, j, off, rank) || rank >= out_cap) continue;
      PeakSums p;
      p.i = base + j;
      const uint64_t kp = v.key(p.i);
      p.m = (uint32_t)(kp >> 32), p.r = (uint32_t)(kp >> 16) & 0xffffu, p.d = (uint32_t)kp & 0xffffu;
      p.cnt = 0;
      p.s = p.sb = p.sr = p.sd = 0.f;
      visit_neighbourhood(v, g, p.i, p.m, p.r, p.d, [&](uint32_t, float mq, int db, int dr, int dd) {
        ++p.cnt;
        p.s += mq;
        p.sb += mq * (float)db;
        p.sr += mq * (float)dr;
        p.sd += mq * (float)dd;
        return true;
      });
      write(rank, v, p);
    }
  }
}

uint32_t run_peaks(const Case& c, bool merge, uint32_t* status, Out& out) {
  const uint32_t* k = c.cfg;
  WalkGeom g;
  if (merge) g = {k[0], k[1], k[2], k[3], k[4], k[5], k[6]};
  else g = {k[0], k[1], 1, 0, k[2], k[3], 0};
  // fmcw_plots.hip / fmcw_merge.hip validate() and the enqueue checks
  REFUSE(g.n_range < 1 || g.n_range > 65536 || g.win_beam > 4 || g.win_range > 4 || g.win_doppler > 4);
  REFUSE(g.n_doppler < 2 * g.win_doppler + 1 || g.n_doppler > 65536 || g.n_beams < 1 || g.n_beams > 64);
  REFUSE(g.beam_wrap > 1 || (g.beam_wrap && g.n_beams < 2 * g.win_beam + 1));
  REFUSE(c.max_recs < 1 || c.max_recs > 0x7fffffffu || c.out_cap > 0x7fffffffu);
  if (merge) {
    REFUSE(c.stride != 16 && c.stride != 32);
    REFUSE(c.max_groups < g.n_beams || c.max_groups % g.n_beams || c.max_groups > 0x7fffffffu);
    REFUSE(c.n_arg > c.max_groups || c.n_arg % g.n_beams);
  } else {
    REFUSE(c.stride != 16);
  }
  const Plan lp = plan_list(c, 1);
  uint8_t* recs = exact<uint8_t>((size_t)lp.cap * c.stride);
  List l = {recs, c.stride, lp.cap, c.n_word, merge ? exact<uint32_t>((size_t)c.n_arg + 1) : nullptr, merge ? c.n_arg : 0u};
  uint64_t* masks = exact<uint64_t>((size_t)lp.tiles * kGroups);
  uint32_t* tile_cnt = exact<uint32_t>(lp.tiles);
  if (c.rec_bytes) memcpy(recs, c.bytes, std::min((size_t)lp.cap * c.stride, (size_t)c.rec_bytes));
  if (lp.tiles) {
    if (merge) frame_index(l), damage_index(l, c.cfg[29]);
    find_peaks(l, g, masks, tile_cnt);
  }
  const uint32_t n_tiles = (in_use(l) + kTile - 1) / kTile;
  const uint32_t bits = lp.tiles ? set_bits(masks, n_tiles) : 0u;
  scan_status(l, tile_cnt, status);
  if (lp.tiles && c.out_cap) {
    if (merge)
      emit_peaks(l, g, masks, tile_cnt, c.out_cap, [&](uint32_t rank, const RecView& v, const PeakSums& p) {
        fmcw_mplot o;
        o.frame = p.m / g.n_beams;
        o.range = (uint16_t)p.r;
        o.doppler = (uint16_t)p.d;
        o.mag = v.mag(p.i);
        o.beam = (uint16_t)(p.m % g.n_beams);
        o.n_merged = (uint16_t)p.cnt;
        o.sum_mag = p.s;
        o.d_beam = p.centre(p.sb);
        o.d_range = p.centre(p.sr);
        o.d_doppler = p.centre(p.sd);
        out.put(rank, o);
      });
    else
      emit_peaks(l, g, masks, tile_cnt, c.out_cap, [&](uint32_t rank, const RecView& v, const PeakSums& p) {
        fmcw_plot o;
        o.frame = p.m;
        o.range = (uint16_t)p.r;
        o.doppler = (uint16_t)p.d;
        o.mag = v.mag(p.i);
        memcpy(&o.threshold, &v.word(p.i)[3], 4);
        o.n_cells = p.cnt;
        o.sum_mag = p.s;
        o.d_range = p.centre(p.sr);
        o.d_doppler = p.centre(p.sd);
        out.put(rank, o);
      });
  }
  free(recs);
  free(l.start);
  free(masks);
  free(tile_cnt);
  return bits;
}

// ---- unfold --------------------------------------------------------------------------------------

struct VList : List {
  uint32_t* vstart;   // n_q + 1 words
  uint32_t n_q, v_cap;
  uint32_t in_use() const {
    const uint32_t n = examined();
    return n ? umin(start[n_groups], n) : 0u;
  }
  uint32_t virtual_len() const { return n_q && examined() ? umin(vstart[n_q], v_cap) : 0u; }
  RecView view() const { return RecView{recs, stride, in_use(), 0, 0, nullptr, nullptr, start}; }
};

// k_unfold_dwells
void dwells(const VList& l, const UnfoldGeom& g) {
  if (!l.examined()) return;
  const RecView rl = l.view();
  for (uint32_t q = 0; q < l.n_q; ++q) {
    uint32_t lo, hi;
    rl.segment(fmcw_unfold::slot_of(g, q).m, lo, hi);
    l.vstart[q] = hi - lo;
  }
  l.vstart[l.n_q] = scan(l.vstart, l.n_q);
}

// unfold_kernel.hpp locate()
bool locate(const VList& l, const UnfoldGeom& g, const RecView& rl, uint32_t v, Slot& s, uint32_t& idx) {
  uint32_t lo = 0, hi = l.n_q - 1;
  while (lo < hi) {
    const uint32_t mid = (lo + hi + 1) >> 1;
    if (l.vstart[mid] <= v) lo = mid;
    else hi = mid - 1;
  }
  s = fmcw_unfold::slot_of(g, lo);
  uint32_t a, b;
  rl.segment(s.m, a, b);
  idx = a + (v - l.vstart[lo]);
  return v >= l.vstart[lo] && idx < b && rl.word(idx)[0] == s.m;
}

uint32_t run_unfold(const Case& c, uint32_t* status, Out& out) {
  const uint32_t* k = c.cfg;
  UnfoldGeom g = {k[0], k[1], k[2], k[11], k[12], k[13], k[14], k[15], k[16], k[17], k[18], k[19], 0, 0};
  // fmcw_unfold.hip validate() and the enqueue checks
  REFUSE(g.n_range < 1 || g.n_range > 65536 || g.tol_range > 4 || g.tol_doppler > 4);
  REFUSE(g.n_doppler < 2 * g.tol_doppler + 1 || g.n_doppler > 65536 || g.n_prf < 2 || g.n_prf > 8);
  uint32_t p_min = 4096;
  for (uint32_t i = 0; i < g.n_prf; ++i) {
    const uint32_t p = k[3 + i];
    REFUSE(p < 1 || p > 4096);
    for (uint32_t j = 0; j < i; ++j) REFUSE(k[3 + j] == p);
    p_min = umin(p_min, p);
    (i < 4 ? g.units_lo : g.units_hi) |= (uint64_t)p << (16 * (i & 3));
  }
  REFUSE(g.prf_phase >= g.n_prf || g.step < 1 || g.step > g.n_prf || g.zero_bin >= g.n_doppler);
  REFUSE(g.v_max > 32ull * g.n_doppler * p_min);
  REFUSE(g.out_unit < 1 || g.out_unit > 65535 || 2ull * g.v_max / g.out_unit + 1 > 65535);
  REFUSE(g.m_of < 1 || g.m_of > g.n_prf || g.n_streams < 1 || g.n_streams > 4096);
  const uint32_t per_rec = (g.n_prf + g.step - 1) / g.step;
  REFUSE(c.max_recs < 1 || (uint64_t)c.max_recs * per_rec > 0x7fffffffull || c.out_cap > 0x7fffffffu);
  REFUSE(c.max_groups < g.n_streams || c.max_groups % g.n_streams || (uint64_t)c.max_groups * g.n_prf > 0x7fffffffull);
  REFUSE(c.stride != 16 && c.stride != 32);
  REFUSE(c.n_arg > c.max_groups / g.n_streams);
  const Plan lp = plan_list(c, per_rec);
  const uint32_t n_scans = c.n_arg;
  const uint32_t n_dwells = n_scans >= g.n_prf ? (n_scans - g.n_prf) / g.step + 1 : 0u;
  VList l;
  l.recs = nullptr, l.stride = c.stride, l.cap = lp.cap, l.n_word = c.n_word;
  l.n_groups = n_scans * g.n_streams;
  l.n_q = n_dwells * g.n_streams * g.n_prf;
  l.v_cap = lp.cap * per_rec;
  uint8_t* recs = exact<uint8_t>((size_t)lp.cap * c.stride);
  if (c.rec_bytes) memcpy(recs, c.bytes, std::min((size_t)lp.cap * c.stride, (size_t)c.rec_bytes));
  l.recs = recs;
  l.start = exact<uint32_t>((size_t)l.n_groups + 1);
  l.vstart = exact<uint32_t>((size_t)l.n_q + 1);
  uint64_t* masks = exact<uint64_t>((size_t)lp.tiles * kGroups);
  uint32_t* tile_cnt = exact<uint32_t>(lp.tiles);
  uint32_t* tie_cnt = exact<uint32_t>(lp.tiles);
  uint32_t* folds = exact<uint32_t>(l.v_cap);
  const bool pairs = lp.tiles && l.n_q;
  if (lp.tiles) frame_index(l), damage_index(l, c.cfg[29]);
  if (pairs) {
    dwells(l, g);
    // k_unfold_find
    const RecView rl = l.view();
    const uint32_t nv = l.virtual_len(), n_tiles = (nv + kTile - 1) / kTile;
    for (uint32_t t = 0; t < n_tiles; ++t) {
      for (uint32_t g2 = 0; g2 < kGroups; ++g2) masks[(size_t)t * kGroups + g2] = 0;
      uint32_t cnt = 0, tie = 0;
      for (uint32_t j = 0; j < kTile; ++j) {
        const uint32_t v = t * kTile + j;
        bool keep = false, tied = false;
        if (v < nv) {
          Slot s;
          uint32_t idx, packed = 0;
          if (locate(l, g, rl, v, s, idx)) {
            const uint32_t rd = rl.word(idx)[1];
            const fmcw_unfold::Verdict w = fmcw_unfold::judge(rl, g, s, idx, rd & 0xffffu, rd >> 16);
            keep = w.report;
            tied = keep && w.n_ties > 1;
            packed = ((uint32_t)w.fold & 0xffffu) | (w.n_ties << 16);
          }
          folds[v] = packed;
        }
        if (keep) set_bit(masks, t, j), ++cnt;
        tie += tied;
      }
      tile_cnt[t] = cnt;
      tie_cnt[t] = tie;
    }
  }
  // k_unfold_scan
  const uint32_t found = l.n_word, n = umin(found, l.cap), use = l.in_use();
  const uint32_t n_tiles = (l.virtual_len() + kTile - 1) / kTile;
  const uint32_t bits = set_bits(masks, n_tiles);
  status[3] = scan(tie_cnt, n_tiles);
  status[0] = scan(tile_cnt, n_tiles);
  status[1] = found - n;
  status[2] = n - use;
  if (pairs && c.out_cap) {
    // k_unfold_emit
    const RecView rl = l.view();
    for (uint32_t t = 0; t < n_tiles; ++t) {
      const uint32_t off = tile_cnt[t];
      if (off >= c.out_cap) break;
      for (uint32_t j = 0; j < kTile; ++j) {
        uint32_t rank;
        if (!rank_of(masks, t, j, off, rank) || rank >= c.out_cap) continue;
        const uint32_t v = t * kTile + j;
        Slot s;
        uint32_t idx;
        if (!locate(l, g, rl, v, s, idx)) continue;
        const uint32_t packed = folds[v];
        out.put(rank, fmcw_unfold::report(rl, g, s, idx, (int)(int16_t)(packed & 0xffffu), packed >> 16));
      }
    }
  }
  free(recs);
  free(l.start);
  free(l.vstart);
  free(masks);
  free(tile_cnt);
  free(tie_cnt);
  free(folds);
  return bits;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) die(2, "usage: reclist_replay CASE RESULT");
  FILE* f = fopen(argv[1], "rb");
  if (!f) die(2, "cannot open the case file");
  uint32_t h[40];
  if (fread(h, 4, 40, f) != 40 || h[0] != 0x50524c52u) die(2, "not a case file");
  Case c;
  c.object = h[1], c.stride = h[2], c.rec_cap = h[3], c.max_recs = h[4], c.n_word = h[5], c.n_arg = h[6];
  c.out_cap = h[7], c.rec_bytes = h[8], c.max_groups = h[9];
  memcpy(c.cfg, h + 10, sizeof(c.cfg));
  std::vector<uint8_t> bytes(c.rec_bytes);
  if (c.rec_bytes && fread(bytes.data(), 1, c.rec_bytes, f) != c.rec_bytes) die(2, "the case file is shorter than rec_bytes");
  fclose(f);
  c.bytes = bytes.data();
  REFUSE(c.object > 2 || c.out_cap > (1u << 24));

  uint32_t status[4] = {kFill, kFill, kFill, kFill};
  Out out = {exact<uint8_t>((size_t)c.out_cap * 32), c.out_cap};
  const uint32_t bits = c.object == 2 ? run_unfold(c, status, out) : run_peaks(c, c.object == 1, status, out);

  const uint32_t r[8] = {0x53524c52u, 2u + c.object, status[0], status[1], status[2], status[3], bits, c.out_cap};
  f = fopen(argv[2], "wb");
  if (!f) die(3, "cannot open the result file");
  if (fwrite(r, 4, 8, f) != 8 || fwrite(out.slots, 32, c.out_cap, f) != c.out_cap || fclose(f)) die(3, "cannot write the result file");
  free(out.slots);
  return 0;
}
