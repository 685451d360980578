// unfold_kernel.hpp -- the velocity unfolder's kernels (fmcw_unfold_*, include/fmcw.h): the beam
// merger's launches over a list in which every (dwell, record) pair has a place of its own.
//
// The output is ordered by (dwell j, stream t, position i, list order), and with step < K a record
// sits in several dwells.  So the kernels do not tile the record list but the virtual list of all
// (dwell, record) pairs in output order: slot q = (j n_streams + t) K + i is frame m(q) = (j step + i)
// n_streams + t, the slots' segments [start[m(q)], start[m(q) + 1]) follow one another, and vstart[q]
// is the virtual index of slot q's first pair.  Tiles, ballot masks and the tile scan run over
// virtual indices, so output order needs no sort and a pair's rank is a popcount, as in the merger.
//
//   k_frame_index    start[m] = the first record whose frame is >= m, for m = 0 .. n_frames (rec_tiles.hpp,
//                    over tiles of the unfolder's shape).  The later launches take
//                    n_use = min(start[n_frames], n) as the list's length.
//   k_unfold_dwells  one workgroup: vstart[q] = exclusive scan of the slots' segment lengths
//                    (tile_offsets_scan), vstart[n_q] = their sum.
//   k_unfold_find    one lane per pair: its slot by a search in vstart, then every hypothesis of the
//                    record in that dwell (unfold_window.hpp judge()).  One 64-bit ballot mask per 64
//                    pairs, per tile the number of reports and of reports with n_ties > 1, and per
//                    pair the best fold and n_ties (4 B), so that emit walks one hypothesis only.
//   k_unfold_scan    one workgroup: exclusive scan of the tile counts (tile_offsets_scan), the sum of the
//                    tie counts, the four status words.
//   k_unfold_emit    rank = tile offset + mask popcounts; the reports below out_cap evaluate their best
//                    hypothesis once more for hit_mask and sum_mag and write their fmcw_vplot.
// A record per lane: the lanes of a wave are neighbours in one frame, so they share the PRF, the
// other scans' segments and, mostly, the number of hypotheses; the searches go to global memory
// (other scans' segments lie whole frames away from the tile, so staging the tile in LDS would serve
// none of them).  Every word a later launch reads (start[0 .. n_frames], vstart[0 .. n_q], the masks,
// counts and folds of the tiles below the virtual length) is written by an earlier launch of the same
// call: nothing to zero between calls, no atomic.
#pragma once
#include "rec_tiles.hpp"
#include "unfold_window.hpp"

namespace fmcw_unfold {

using fmcw_rec::RecList;
using fmcw_rec::examined;

// 16 waves: a lane's work is a chain of dependent searches, so a tile's pairs run side by side (4 per
// lane in turn took 265 us, not 96, on a short list)
using UnfoldTiles = fmcw_rec::Tiles<1024, 1>;
constexpr uint32_t kMaxGrid = 4096;          // workgroups of index / find / emit (they stride over the tiles)
constexpr int kScanThreads = 1024;

// What one call reads its list through; by value to every kernel.
struct UnfoldList : RecList {  // start: n_frames + 1 words, n_groups = n_frames = n_scans n_streams
  const uint32_t* vstart;      // n_q + 1 words
  uint32_t n_q;                // n_dwells n_streams K
  uint32_t v_cap;              // cap ceil(K / step): what the per-pair scratch holds
};

// The records that take part: those below frame n_frames.  Not rec_tiles.hpp's in_use() and scan_status(): the
// unfolder always has an index, and their test for a list without one (a branch in every kernel's
// prologue, the status words no longer one store in the one-workgroup scan) cost it 0.5 - 1 % per call.
__device__ __forceinline__ uint32_t in_use(const UnfoldList& l) {
  const uint32_t n = examined(l);
  return n ? min(l.start[l.n_groups], n) : 0u;
}
// the (dwell, record) pairs; an ordered list never reaches v_cap
__device__ __forceinline__ uint32_t virtual_len(const UnfoldList& l) {
  return l.n_q && examined(l) ? min(l.vstart[l.n_q], l.v_cap) : 0u;
}
// the records that take part, read in place
__device__ __forceinline__ RecView rec_view(const UnfoldList& l) {
  return RecView{l.recs, l.stride, in_use(l), 0, 0, nullptr, nullptr, l.start};
}

// One workgroup: the slots' segment lengths, scanned in place.  vstart holds max_frames K + 1 words.
__global__ void __launch_bounds__(kScanThreads) k_unfold_dwells(UnfoldList l, UnfoldGeom g, uint32_t* __restrict__ vstart) {
  if (!examined(l)) return;                     // nothing reads vstart[] then
  const RecView rl = rec_view(l);
  for (uint32_t q = threadIdx.x; q < l.n_q; q += kScanThreads) {
    uint32_t lo, hi;
    rl.segment(slot_of(g, q).m, lo, hi);
    vstart[q] = hi - lo;
  }
  __syncthreads();
  const uint32_t sum = fmcw::tile_offsets_scan<kScanThreads>(vstart, vstart, (int)l.n_q);
  if (threadIdx.x == 0) vstart[l.n_q] = sum;
}

// The slot and the record of virtual index v < virtual_len; false where the index does not hold up
// (an unordered list): such a pair is never a report and indexes nothing.
__device__ __forceinline__ bool locate(const UnfoldList& l, const UnfoldGeom& g, const RecView& rl, uint32_t v, Slot& s,
                                       uint32_t& idx) {
  uint32_t lo = 0, hi = l.n_q - 1;              // the last slot whose vstart is <= v
  while (lo < hi) {
    const uint32_t mid = (lo + hi + 1) >> 1;
    if (l.vstart[mid] <= v) lo = mid;
    else hi = mid - 1;
  }
  s = slot_of(g, lo);
  uint32_t a, b;
  rl.segment(s.m, a, b);
  idx = a + (v - l.vstart[lo]);
  return v >= l.vstart[lo] && idx < b && rl.word(idx)[0] == s.m;
}

__global__ void __launch_bounds__(UnfoldTiles::kThreads) k_unfold_find(UnfoldList l, UnfoldGeom g,
                                                                        uint64_t* __restrict__ masks,
                                                                        uint32_t* __restrict__ tile_cnt,
                                                                        uint32_t* __restrict__ tie_cnt,
                                                                        uint32_t* __restrict__ folds) {
  using T = UnfoldTiles;
  __shared__ uint32_t s_cnt[T::kGroups], s_tie[T::kGroups];
  const RecView rl = rec_view(l);
  const uint32_t nv = virtual_len(l);
  const uint32_t n_tiles = T::count(nv);
  for (uint32_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    for (int k = 0; k < T::kPer; ++k) {
      const uint32_t v = t * T::kTile + k * T::kThreads + threadIdx.x;
      bool keep = false, tied = false;
      if (v < nv) {
        Slot s;
        uint32_t idx;
        uint32_t packed = 0;
        if (locate(l, g, rl, v, s, idx)) {
          const uint32_t rd = rl.word(idx)[1];
          const Verdict w = judge(rl, g, s, idx, rd & 0xffffu, rd >> 16);
          keep = w.report;
          tied = keep && w.n_ties > 1;
          packed = ((uint32_t)w.fold & 0xffffu) | (w.n_ties << 16);
        }
        folds[v] = packed;                      // v < v_cap
      }
      T::put(__ballot(keep), t, k, masks, s_cnt);
      T::tally(__ballot(tied), k, s_tie);
    }
    __syncthreads();
    T::sum(s_cnt, &tile_cnt[t]);
    T::sum(s_tie, &tie_cnt[t]);
    __syncthreads();   // before the next tile's lanes overwrite the group counts
  }
}

// One workgroup: tile_cnt -> exclusive scan in place, the tie counts' sum, and the status words.
__global__ void __launch_bounds__(kScanThreads) k_unfold_scan(UnfoldList l, uint32_t* __restrict__ tile_cnt,
                                                               uint32_t* __restrict__ tie_cnt, uint32_t* __restrict__ status) {
  const uint32_t found = l.n_recs[0];
  const uint32_t n = min(found, l.cap);
  const uint32_t use = in_use(l);
  const int n_tiles = (int)UnfoldTiles::count(virtual_len(l));   // < 2^21, a tile has at most kTile reports
  const uint32_t ties = fmcw::tile_offsets_scan<kScanThreads>(tie_cnt, tie_cnt, n_tiles);   // only the sum is used
  const uint32_t sum = fmcw::tile_offsets_scan<kScanThreads>(tile_cnt, tile_cnt, n_tiles);
  if (threadIdx.x == 0) {
    status[0] = sum;
    status[1] = found - n;
    status[2] = n - use;
    status[3] = ties;
  }
}

__global__ void __launch_bounds__(UnfoldTiles::kThreads) k_unfold_emit(UnfoldList l, UnfoldGeom g,
                                                                        const uint64_t* __restrict__ masks,
                                                                        const uint32_t* __restrict__ tile_off,
                                                                        const uint32_t* __restrict__ folds,
                                                                        fmcw_vplot* __restrict__ out, uint32_t out_cap) {
  using T = UnfoldTiles;
  __shared__ uint64_t s_m[T::kGroups];
  const RecView rl = rec_view(l);
  const uint32_t n_tiles = T::count(virtual_len(l));
  for (uint32_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const uint32_t off = tile_off[t];
    if (off >= out_cap) break;  // offsets only grow with t: nothing left to write for this workgroup
    __syncthreads();
    T::load_masks(masks, t, s_m);
    __syncthreads();
    for (int k = 0; k < T::kPer; ++k) {
      uint32_t rank;
      if (!T::rank(s_m, k, off, rank) || rank >= out_cap) continue;
      const uint32_t v = t * T::kTile + k * T::kThreads + threadIdx.x;
      Slot s;
      uint32_t idx;
      if (!locate(l, g, rl, v, s, idx)) continue;   // find kept it, so this holds
      const uint32_t packed = folds[v];
      out[rank] = report(rl, g, s, idx, (int)(int16_t)(packed & 0xffffu), packed >> 16);
    }
  }
}

}  // namespace fmcw_unfold
