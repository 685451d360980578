// merge_kernel.hpp -- the beam merger's kernels (fmcw_merge_*, include/fmcw.h): the plot extractor's
// three launches behind a map index, with the beam as a third axis of the neighbourhood.  All four are
// the shared list layer (rec_tiles.hpp, rec_window.hpp) with the merger's tile shape and record.
//
//   k_frame_index  start[m] = the first record whose frame is >= m, for m = 0 .. n_maps.  The later
//                  launches take n_use = min(start[n_maps], n) as the list's length, which is how the
//                  records at or beyond frame n_maps are never a peak, never a neighbour and never
//                  index anything.
//   k_merge_find   find_peaks: one ballot mask per 64 records, one peak count per tile.
//   k_merge_scan   one workgroup: exclusive scan of the tile counts and the three status words.
//   k_merge_emit   emit_peaks: the peaks below out_cap write their fmcw_mplot.
// Every word a later launch reads (start[0 .. n_maps], the masks and counts of the tiles below n_use)
// is written by an earlier launch of the same call: nothing to zero between calls, no atomic.
#pragma once
#include "rec_tiles.hpp"

namespace fmcw_merge {

using namespace fmcw_rec;

using MergeTiles = Tiles<256, 4>;            // 4 waves, 4 records per lane and tile
constexpr uint32_t kHalo = 512;              // staged either side of the tile
constexpr uint32_t kMaxGrid = 4096;          // workgroups of index / find / emit (they stride over the tiles)
constexpr int kScanThreads = 1024;

__global__ void __launch_bounds__(MergeTiles::kThreads) k_merge_find(RecList l, WalkGeom g, uint64_t* __restrict__ masks,
                                                                      uint32_t* __restrict__ tile_cnt) {
  find_peaks<MergeTiles, kHalo>(l, g, masks, tile_cnt);
}

__global__ void __launch_bounds__(kScanThreads) k_merge_scan(RecList l, uint32_t* __restrict__ tile_cnt,
                                                              uint32_t* __restrict__ status) {
  scan_status<kScanThreads>(l, tile_cnt, MergeTiles::count(in_use(l)), status);
}

__global__ void __launch_bounds__(MergeTiles::kThreads) k_merge_emit(RecList l, WalkGeom g, const uint64_t* __restrict__ masks,
                                                                      const uint32_t* __restrict__ tile_off,
                                                                      fmcw_mplot* __restrict__ out, uint32_t out_cap) {
  emit_peaks<MergeTiles, kHalo>(l, g, masks, tile_off, out_cap, [&](uint32_t rank, const RecView& v, const PeakSums& p) {
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
    out[rank] = o;
  });
}

}  // namespace fmcw_merge
