// rec_tiles.hpp -- the tile machinery that the kernels over an ordered record list share (plot
// extractor, beam merger, velocity unfolder, and the device tracker for the index): the list as a
// kernel argument, the frame index, the ballot masks / counts / ranks of a tile, the staging of a tile
// in LDS, the status words of the scan launch, and the find and emit passes of the two peak groupers.
// Device code; what one lane does with the list is rec_window.hpp.
//
// The pattern is three launches, with no atomic and no word that outlives a call: a find pass leaves
// one 64-bit ballot mask per 64 items and one count per tile, one workgroup scans the counts
// (det_sink.hpp tile_offsets_scan) and writes the status words, and an emit pass ranks every kept item
// by tile offset + mask popcounts, so the output keeps list order.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "det_sink.hpp"
#include "rec_window.hpp"

namespace fmcw_rec {

// What one call reads its list through; by value to every kernel.  start = nullptr: no frame index,
// every examined record takes part (the plot extractor).
struct RecList {
  const uint8_t* recs;
  uint32_t stride, cap;        // cap = min(rec_cap, the object's max_recs)
  const uint32_t* n_recs;
  const uint32_t* start;       // n_groups + 1 words
  uint32_t n_groups;           // frames that take part
};

__device__ __forceinline__ uint32_t examined(const RecList& l) { return min(l.n_recs[0], l.cap); }
// the records that take part: those below frame n_groups
__device__ __forceinline__ uint32_t in_use(const RecList& l) {
  const uint32_t n = examined(l);
  return n && l.start ? min(l.start[l.n_groups], n) : n;
}

// start[m] = the first record whose frame is >= m, for m = 0 .. n_groups.  Item i (0 .. n, one more
// than the records) compares frame[i-1] and frame[i] (frame[-1] "before 0", frame[n] "after the
// last") and writes start[m] = i for every m in (frame[i-1], min(frame[i], n_groups)]: empty frames and
// the gaps before the first and after the last record come out of the same store loop.  Only the frame
// word of a record is read.  The list is ordered, so the records at or beyond frame n_groups are the
// suffix from start[n_groups].  Persistent over tiles of Threads x Per items; the grid covers
// cap / tile + 1 tiles, one more than the records' when cap is a multiple of the tile.  SkipEmpty:
// nothing reads start[] after an empty list; without it item 0 writes start[0 .. n_groups] = 0.
// A template, so that every translation unit that includes this header may define it.
template <int Threads, int Per, bool SkipEmpty>
__global__ void __launch_bounds__(Threads) k_frame_index(const uint8_t* __restrict__ recs, uint32_t stride,
                                                          uint32_t cap, const uint32_t* __restrict__ n_recs,
                                                          uint32_t n_groups, uint32_t* __restrict__ start) {
  constexpr uint32_t kTile = Threads * Per;
  const uint32_t n = min(n_recs[0], cap);   // cap < 2^31: n + 1 items fit 32 bits
  if (SkipEmpty && !n) return;
  const uint32_t n_tiles = n / kTile + 1;   // ceil((n + 1) / kTile)
  const int64_t G = (int64_t)n_groups;
  for (uint32_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    for (int k = 0; k < Per; ++k) {
      const uint32_t i = t * kTile + (uint32_t)k * Threads + threadIdx.x;
      if (i > n) continue;
      const int64_t prev = i ? (int64_t) * reinterpret_cast<const uint32_t*>(recs + (size_t)(i - 1) * stride) : -1;
      int64_t cur = G;
      if (i < n) cur = min((int64_t) * reinterpret_cast<const uint32_t*>(recs + (size_t)i * stride), G);
      for (int64_t m = prev + 1; m <= cur; ++m) start[m] = i;   // 0 <= m <= n_groups: start holds n_groups + 1 words at least
    }
  }
}

// A tile is Threads x Per consecutive items; lane `tid` owns items base + k Threads + tid, k < Per, and
// the 64 items of wave w's k-th turn are group k (Threads / 64) + w: groups ascend in item order.
template <int Threads, int Per>
struct Tiles {
  static constexpr int kThreads = Threads, kPer = Per;
  static constexpr uint32_t kTile = Threads * Per;
  static constexpr int kGroups = kTile / 64;   // ballot masks per tile

  static __device__ __forceinline__ uint32_t count(uint32_t n) { return (n + kTile - 1) / kTile; }
  static __device__ __forceinline__ uint32_t group(int k) { return k * (Threads / 64) + (threadIdx.x >> 6); }

  // Lane 0 of each wave, with the ballot of the lanes' flags for their k-th item: the group's count
  // into s_cnt.  (The ballot is taken by the caller: taken in here from a bool argument, the find
  // kernels come out a tenth longer, with SGPRs spilled.)
  static __device__ __forceinline__ void tally(uint64_t mk, int k, uint32_t* s_cnt) {
    if ((threadIdx.x & 63) == 0) s_cnt[group(k)] = (uint32_t)__popcll(mk);
  }
  // tally(), and the ballot into tile t's masks
  static __device__ __forceinline__ void put(uint64_t mk, uint32_t t, int k, uint64_t* masks, uint32_t* s_cnt) {
    if ((threadIdx.x & 63) == 0) {
      masks[(size_t)t * kGroups + group(k)] = mk;
      s_cnt[group(k)] = (uint32_t)__popcll(mk);
    }
  }
  // after a __syncthreads() behind the tile's put() / tally() calls: *tile_cnt = the sum of the group counts
  static __device__ __forceinline__ void sum(const uint32_t* s_cnt, uint32_t* tile_cnt) {
    if (threadIdx.x == 0) {
      uint32_t c = 0;
      for (int j = 0; j < kGroups; ++j) c += s_cnt[j];
      *tile_cnt = c;
    }
  }
  // tile t's masks into s_m; the caller syncs after it
  static __device__ __forceinline__ void load_masks(const uint64_t* __restrict__ masks, uint32_t t, uint64_t* s_m) {
    if (threadIdx.x < kGroups) s_m[threadIdx.x] = masks[(size_t)t * kGroups + threadIdx.x];
  }
  // Whether this lane's k-th item is kept, and then its rank: off + the kept items before it in the tile.
  static __device__ __forceinline__ bool rank(const uint64_t* s_m, int k, uint32_t off, uint32_t& rank) {
    const int grp = (int)group(k);
    const uint32_t lane = threadIdx.x & 63;
    rank = off;
    for (int j = 0; j < grp; ++j) rank += (uint32_t)__popcll(s_m[j]);
    const uint64_t mk = s_m[grp];
    rank += (uint32_t)__popcll(mk & ((1ull << lane) - 1ull));
    return (mk >> lane) & 1ull;
  }
};

// The view of the list's first n records with tile `base`'s span staged as (64-bit key, magnitude),
// kHalo records either side of the tile; every lane of the workgroup calls it and the caller syncs
// after it.  s_key and s_mag hold T::kTile + 2 kHalo entries.
template <class T, uint32_t kHalo>
__device__ __forceinline__ RecView stage_tile(const RecList& l, uint32_t n, uint32_t base, uint64_t* s_key, float* s_mag) {
  RecView v;
  v.recs = l.recs;
  v.stride = l.stride;
  v.n = n;
  v.s_lo = base > kHalo ? base - kHalo : 0u;
  v.s_n = min(n, base + T::kTile + kHalo) - v.s_lo;  // <= kTile + 2 kHalo (base < n)
  v.s_key = s_key;
  v.s_mag = s_mag;
  v.start = l.start;
  for (uint32_t j = threadIdx.x; j < v.s_n; j += T::kThreads) {
    const uint32_t* p = v.word(v.s_lo + j);
    const uint32_t rd = p[1];
    s_key[j] = make_key(p[0], rd & 0xffffu, rd >> 16);
    s_mag[j] = __uint_as_float(p[2]);
  }
  return v;
}

// The tail of a scan launch (one workgroup of ScanThreads): tile_cnt[0 .. n_tiles) -> its exclusive scan
// in place; status[0] = the sum, status[1] = records not examined and, where there is an index,
// status[2] = records at or beyond frame n_groups.  n_tiles < 2^21 and a tile keeps at most its items.
template <int ScanThreads>
__device__ __forceinline__ void scan_status(const RecList& l, uint32_t* tile_cnt, uint32_t n_tiles, uint32_t* status) {
  const uint32_t found = l.n_recs[0];
  const uint32_t n = min(found, l.cap);
  const uint32_t use = in_use(l);
  const uint32_t sum = fmcw::tile_offsets_scan<ScanThreads>(tile_cnt, tile_cnt, (int)n_tiles);
  if (threadIdx.x == 0) {
    status[0] = sum;
    status[1] = found - n;
    if (l.start) status[2] = n - use;
  }
}

// The find pass of a peak grouper: one lane per record, the tile staged with its halo; the peak test
// over the neighbourhood stops at the first larger neighbour (ties go to the first in list order).
// Probes of the record's own map mostly hit the staged span; another beam's map lies a whole map
// further on and is read in place.
template <class T, uint32_t kHalo>
__device__ __forceinline__ void find_peaks(const RecList& l, const WalkGeom& g, uint64_t* __restrict__ masks,
                                           uint32_t* __restrict__ tile_cnt) {
  __shared__ uint64_t s_key[T::kTile + 2 * kHalo];
  __shared__ float s_mag[T::kTile + 2 * kHalo];
  __shared__ uint32_t s_cnt[T::kGroups];
  const uint32_t n = in_use(l);
  const uint32_t n_tiles = T::count(n);
  for (uint32_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const uint32_t base = t * T::kTile;
    __syncthreads();  // the previous tile's readers are done with the staging arrays and the counts
    const RecView v = stage_tile<T, kHalo>(l, n, base, s_key, s_mag);
    __syncthreads();
    for (int k = 0; k < T::kPer; ++k) {
      const uint32_t i = base + k * T::kThreads + threadIdx.x;
      bool peak = false;
      if (i < n) {
        const uint64_t kp = v.key(i);
        const float mp = v.mag(i);
        // an ordered list has no frame >= n_groups below n; an unordered one must still not index start[] past its end
        peak = !l.start || (uint32_t)(kp >> 32) < l.n_groups;
        if (peak) visit_neighbourhood(v, g, i, (uint32_t)(kp >> 32), (uint32_t)(kp >> 16) & 0xffffu, (uint32_t)kp & 0xffffu,
                            [&](uint32_t q, float mq, int, int, int) {
                              if (q != i && (mq > mp || (mq == mp && q < i))) peak = false;
                              return peak;
                            });
      }
      T::put(__ballot(peak), t, k, masks, s_cnt);
    }
    __syncthreads();
    T::sum(s_cnt, &tile_cnt[t]);
  }
}

// What the emit pass of a peak grouper hands to its record writer: peak i = (frame m, r, d) of view v,
// the records of its neighbourhood (itself included) and the magnitude sums over them, plain and
// weighted by the beam, range and Doppler offset; centre(x) is x / s where s is finite and not zero.
struct PeakSums {
  uint32_t i, m, r, d, cnt;
  float s, sb, sr, sd;
  FMCW_HD float centre(float x) const {
    return s != 0.f && fabsf(s) <= 3.402823466e38f ? x / s : 0.f;   // NaN compares false
  }
};

// The emit pass of a peak grouper: only the peaks below out_cap walk their neighbourhood again, for the
// sums, and write(rank, v, sums) stores the record.
template <class T, uint32_t kHalo, class W>
__device__ __forceinline__ void emit_peaks(const RecList& l, const WalkGeom& g, const uint64_t* __restrict__ masks,
                                           const uint32_t* __restrict__ tile_off, uint32_t out_cap, W&& write) {
  __shared__ uint64_t s_key[T::kTile + 2 * kHalo];
  __shared__ float s_mag[T::kTile + 2 * kHalo];
  __shared__ uint64_t s_m[T::kGroups];
  const uint32_t n = in_use(l);
  const uint32_t n_tiles = T::count(n);
  for (uint32_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const uint32_t base = t * T::kTile;
    const uint32_t off = tile_off[t];
    if (off >= out_cap) break;  // offsets only grow with t: nothing left to write for this workgroup
    __syncthreads();
    const RecView v = stage_tile<T, kHalo>(l, n, base, s_key, s_mag);
    T::load_masks(masks, t, s_m);
    __syncthreads();
    for (int k = 0; k < T::kPer; ++k) {
      uint32_t rank;
      if (!T::rank(s_m, k, off, rank) || rank >= out_cap) continue;
      PeakSums p;
      p.i = base + k * T::kThreads + threadIdx.x;
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

}  // namespace fmcw_rec
