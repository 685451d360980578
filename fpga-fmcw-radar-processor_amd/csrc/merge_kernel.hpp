// merge_kernel.hpp -- the beam merger's kernels (fmcw_merge_*, include/fmcw.h): the plot extractor's
// three launches behind a map index, with the beam as a third axis of the neighbourhood.
//
//   k_merge_index  start[m] = the first record whose frame is >= m, for m = 0 .. n_maps.  Item i (0 .. n,
//                  one more than the records) compares frame[i-1] and frame[i] (frame[-1] "before 0",
//                  frame[n] "after the last") and writes start[m] = i for every m in (frame[i-1],
//                  min(frame[i], n_maps)]: empty maps and the gaps before the first and after the last
//                  record come out of the same store loop.  The list is ordered, so the records at or
//                  beyond frame n_maps are the suffix from start[n_maps]; the later launches take
//                  n_use = min(start[n_maps], n) as the list's length, which is how those records are
//                  never a peak, never a neighbour and never index anything.
//                  This is k_tws_index of tws_dev_kernel.hpp restated: that header defines its kernels
//                  as plain (non-inline, non-template) __global__ functions next to the tracker's, so a
//                  second translation unit that includes it defines them a second time.
//   k_merge_find   one lane per record, kTile-record tiles staged in LDS with kHalo records either side
//                  as (64-bit key, magnitude); the peak test over the neighbourhood (merge_window.hpp)
//                  stops at the first larger neighbour.  One 64-bit ballot mask per 64 records, one peak
//                  count per tile.  Probes of the record's own map mostly hit the staged span; another
//                  beam's map lies a whole map further on and is read in place.
//   k_merge_scan   one workgroup: exclusive scan of the tile counts (det_sink.hpp tile_offsets_scan)
//                  and the three status words.
//   k_merge_emit   rank = tile offset + mask popcounts; only peaks below out_cap walk their
//                  neighbourhood again, for the sums, and write their fmcw_mplot.
// Every word a later launch reads (start[0 .. n_maps], the masks and counts of the tiles below n_use)
// is written by an earlier launch of the same call: nothing to zero between calls, no atomic.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "det_sink.hpp"
#include "merge_window.hpp"

namespace fmcw_merge {

constexpr int kThreads = 256;                // 4 waves
constexpr int kPer = 4;                      // records per lane and tile
constexpr uint32_t kTile = kThreads * kPer;  // records per tile
constexpr uint32_t kHalo = 512;              // staged either side of the tile
constexpr uint32_t kStage = kTile + 2 * kHalo;
constexpr int kGroups = kTile / 64;          // ballot masks per tile
constexpr uint32_t kMaxGrid = 4096;          // workgroups of index / find / emit (they stride over the tiles)
constexpr int kScanThreads = 1024;

// What one call reads its list through; by value to every kernel.
struct MergeList {
  const uint8_t* recs;
  uint32_t stride, cap;        // cap = min(rec_cap, max_recs)
  const uint32_t* n_recs;
  const uint32_t* start;
  uint32_t n_maps;
};

__device__ __forceinline__ uint32_t examined(const MergeList& l) { return min(l.n_recs[0], l.cap); }
// the records that take part: those below frame n_maps
__device__ __forceinline__ uint32_t in_use(const MergeList& l) {
  const uint32_t n = examined(l);
  return n ? min(l.start[l.n_maps], n) : 0u;
}

__global__ void __launch_bounds__(kThreads) k_merge_index(MergeList l, uint32_t* __restrict__ start) {
  const uint32_t n = examined(l);
  if (!n) return;                               // nothing reads start[] then
  const uint32_t n_tiles = n / kTile + 1;       // ceil((n + 1) / kTile)
  const int64_t G = (int64_t)l.n_maps;
  for (uint32_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    for (int k = 0; k < kPer; ++k) {
      const uint32_t i = t * kTile + (uint32_t)k * kThreads + threadIdx.x;
      if (i > n) continue;
      const int64_t prev = i ? (int64_t) * reinterpret_cast<const uint32_t*>(l.recs + (size_t)(i - 1) * l.stride) : -1;
      int64_t cur = G;
      if (i < n) cur = min((int64_t) * reinterpret_cast<const uint32_t*>(l.recs + (size_t)i * l.stride), G);
      for (int64_t m = prev + 1; m <= cur; ++m) start[m] = i;   // 0 <= m <= n_maps: start holds max_maps + 1 words
    }
  }
}

// Stage tile t's span; every lane of the workgroup calls it.  The caller syncs after it.
__device__ __forceinline__ RecView stage_tile(const MergeList& l, uint32_t n, uint32_t base, uint64_t* s_key,
                                              float* s_mag) {
  RecView v;
  v.recs = l.recs;
  v.stride = l.stride;
  v.n = n;
  v.s_lo = base > kHalo ? base - kHalo : 0u;
  v.s_n = min(n, base + kTile + kHalo) - v.s_lo;  // <= kStage (base < n)
  v.s_key = s_key;
  v.s_mag = s_mag;
  v.start = l.start;
  for (uint32_t j = threadIdx.x; j < v.s_n; j += kThreads) {
    const uint32_t* p = v.word(v.s_lo + j);
    const uint32_t rd = p[1];
    s_key[j] = make_key(p[0], rd & 0xffffu, rd >> 16);
    s_mag[j] = __uint_as_float(p[2]);
  }
  return v;
}

__global__ void __launch_bounds__(kThreads) k_merge_find(MergeList l, MergeGeom g, uint64_t* __restrict__ masks,
                                                          uint32_t* __restrict__ tile_cnt) {
  __shared__ uint64_t s_key[kStage];
  __shared__ float s_mag[kStage];
  __shared__ uint32_t s_cnt[kGroups];
  const uint32_t n = in_use(l);
  const uint32_t n_tiles = (n + kTile - 1) / kTile;
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (uint32_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const uint32_t base = t * kTile;
    __syncthreads();  // the previous tile's readers are done with the staging arrays
    const RecView v = stage_tile(l, n, base, s_key, s_mag);
    __syncthreads();
    for (int k = 0; k < kPer; ++k) {
      const uint32_t i = base + k * kThreads + tid;
      bool peak = false;
      if (i < n) {
        const uint64_t kp = v.key(i);
        const float mp = v.mag(i);
        // an ordered list has no frame >= n_maps below n; an unordered one must still not index start[] past its end
        peak = (uint32_t)(kp >> 32) < l.n_maps;
        if (peak) visit_neighbourhood(v, g, i, (uint32_t)(kp >> 32), (uint32_t)(kp >> 16) & 0xffffu, (uint32_t)kp & 0xffffu,
                            [&](uint32_t q, float mq, int, int, int) {
                              if (q != i && (mq > mp || (mq == mp && q < i))) peak = false;
                              return peak;
                            });
      }
      const uint64_t mk = __ballot(peak);
      if (lane == 0) {
        masks[(size_t)t * kGroups + k * (kThreads / 64) + wave] = mk;
        s_cnt[k * (kThreads / 64) + wave] = (uint32_t)__popcll(mk);
      }
    }
    __syncthreads();
    if (tid == 0) {
      uint32_t c = 0;
      for (int j = 0; j < kGroups; ++j) c += s_cnt[j];
      tile_cnt[t] = c;
    }
  }
}

// One workgroup: tile_cnt -> exclusive scan in place, and the status words.
__global__ void __launch_bounds__(kScanThreads) k_merge_scan(MergeList l, uint32_t* __restrict__ tile_cnt,
                                                              uint32_t* __restrict__ status) {
  const uint32_t found = l.n_recs[0];
  const uint32_t n = min(found, l.cap);
  const uint32_t use = in_use(l);
  const uint32_t n_tiles = (use + kTile - 1) / kTile;   // <= 2^21, a tile has at most kTile peaks
  const uint32_t sum = fmcw::tile_offsets_scan<kScanThreads>(tile_cnt, tile_cnt, (int)n_tiles);
  if (threadIdx.x == 0) {
    status[0] = sum;
    status[1] = found - n;
    status[2] = n - use;
  }
}

__global__ void __launch_bounds__(kThreads) k_merge_emit(MergeList l, MergeGeom g, const uint64_t* __restrict__ masks,
                                                          const uint32_t* __restrict__ tile_off,
                                                          fmcw_mplot* __restrict__ out, uint32_t out_cap) {
  __shared__ uint64_t s_key[kStage];
  __shared__ float s_mag[kStage];
  __shared__ uint64_t s_m[kGroups];
  const uint32_t n = in_use(l);
  const uint32_t n_tiles = (n + kTile - 1) / kTile;
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (uint32_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const uint32_t base = t * kTile;
    const uint32_t off = tile_off[t];
    if (off >= out_cap) break;  // offsets only grow with t: nothing left to write for this workgroup
    __syncthreads();
    const RecView v = stage_tile(l, n, base, s_key, s_mag);
    if (tid < kGroups) s_m[tid] = masks[(size_t)t * kGroups + tid];
    __syncthreads();
    for (int k = 0; k < kPer; ++k) {
      const int grp = k * (kThreads / 64) + (int)wave;  // records base + 64 grp ..: list order
      uint32_t rank = off;
      for (int j = 0; j < grp; ++j) rank += (uint32_t)__popcll(s_m[j]);
      const uint64_t mk = s_m[grp];
      rank += (uint32_t)__popcll(mk & ((1ull << lane) - 1ull));
      const uint32_t i = base + k * kThreads + tid;
      if (!((mk >> lane) & 1ull) || rank >= out_cap) continue;
      const uint64_t kp = v.key(i);
      const uint32_t m = (uint32_t)(kp >> 32), r = (uint32_t)(kp >> 16) & 0xffffu, d = (uint32_t)kp & 0xffffu;
      uint32_t cnt = 0;
      float s = 0.f, sb = 0.f, sr = 0.f, sd = 0.f;
      visit_neighbourhood(v, g, i, m, r, d, [&](uint32_t, float mq, int db, int dr, int dd) {
        ++cnt;
        s += mq;
        sb += mq * (float)db;
        sr += mq * (float)dr;
        sd += mq * (float)dd;
        return true;
      });
      const bool ok = s != 0.f && fabsf(s) <= 3.402823466e38f;  // finite (NaN compares false)
      fmcw_mplot o;
      o.frame = m / g.n_beams;
      o.range = (uint16_t)r;
      o.doppler = (uint16_t)d;
      o.mag = v.mag(i);
      o.beam = (uint16_t)(m % g.n_beams);
      o.n_merged = (uint16_t)cnt;
      o.sum_mag = s;
      o.d_beam = ok ? sb / s : 0.f;
      o.d_range = ok ? sr / s : 0.f;
      o.d_doppler = ok ? sd / s : 0.f;
      out[rank] = o;
    }
  }
}

}  // namespace fmcw_merge
