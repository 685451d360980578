// tws_dev_kernel.hpp -- the device track-while-scan tracker's kernels (fmcw_tws_dev_*, include/fmcw.h).
//
// The arithmetic is csrc/tws_tracker.cpp's fmcw_tws_scan, statement for statement (the same helpers
// wrap / resize_s / floor_shr8 over 64-bit integers in both modes, so there is no bound to argue: a
// track that coasts for coast_max = 2^32 - 1 scans moves its position past 32 bits on the host too).
//
//   k_frame_index start[g] = the first record whose frame is >= g, for g = 0 .. G (G = n_scans *
//                 n_streams): the shared index of rec_tiles.hpp over tiles of kIdxTile = 1024 items, here
//                 also for an empty list (every start word is 0 then).  Because the list is ordered,
//                 the records at or beyond frame G are the suffix from start[G]: the tracker kernel
//                 reports n - start[G] as status word 1, so no counter has to be zeroed between calls.
//   k_tws_track   one wave64 per workgroup and per stream (s = blockIdx.x; s += gridDim.x), serial over
//                 the scans.  Lane t owns track slot t (state in registers across the scans, loaded from
//                 and stored to the handle's state block around a stream's run); lane i holds detection
//                 i of the current scan.  One wave per workgroup: the waves never share anything, and a
//                 workgroup of one wave lets the dispatcher spread 64 streams over 64 CUs instead of 16.
//                 The next scan's records are loaded before the current scan is worked on, and the
//                 start words one scan before that, so neither load's latency is on the serial chain.
//     PREDICT, UPDATE, MAINTAIN, OUTPUT   lane-parallel over the tracks.
//     ASSOCIATE   serial over the set bits of the active-track ballot (the claimed flags are order
//                 dependent).  The track's predicted position is broadcast (v_readlane), every lane forms
//                 its detection's gate test and |dr| + |dd|.  Intended mode: one wave-minimum (DPP row
//                 shifts and broadcasts) over the key dist * 64 + lane gives the nearest detection, the
//                 lowest index on ties; dist < 2 * 4 * 4096, so the key fits 21 bits.  RTL mode: one
//                 ballot of the candidates compared against the best_distance the previous active track
//                 left; the highest candidate lane wins (the last qualifying detection).
//                 A track's UPDATE touches only that track and no later association reads it, so the
//                 loop only records (hit, detection index) in the track's lane; UPDATE follows the loop.
//     INITIATE    the k-th unclaimed detection goes to the k-th free slot: two ballots, a prefix
//                 popcount on the slot side and a select-k-th-set-bit on the detection side.
//     OUTPUT      firm and coasting slots compacted by ballot prefix; an fmcw_track is written as seven
//                 dword stores.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/fmcw.h"
#include "rec_tiles.hpp"

namespace fmcw_twsd {

constexpr int kIdxThreads = 256;
constexpr int kIdxPer = 4;
constexpr uint32_t kIdxTile = kIdxThreads * kIdxPer;   // items per tile
constexpr uint32_t kIdxMaxGrid = 1024;                  // workgroups of the index at most
constexpr uint32_t kTrackMaxGrid = 4096;                // workgroups (waves) of k_tws_track at most
constexpr uint32_t kMaxRecs = 0x7fffffffu;              // n + 1 items fit 32 bits

// Per-stream state block: kStateFields rows of 64 words, row f lane t = field f of slot t.
enum {
  S_RP_LO, S_RP_HI, S_DP_LO, S_DP_HI, S_RV_LO, S_RV_HI, S_DV_LO, S_DV_HI,
  S_HIT, S_MISS, S_QUALITY, S_AGE, S_LAST_MAG, S_FLAGS,   // flags: bit 0 active, bits 1..2 status
  S_BEST,                                                  // lane 0 best_distance, lane 1 best_idx
  kStateFields
};
constexpr uint32_t kStateWords = kStateFields * 64;
constexpr uint32_t kBestDistancePowerUp = 0xFFFF, kBestIdxPowerUp = 63;   // tws_tracker.vhd:92-93

enum { T_FREE = 0, T_TENT = 1, T_FIRM = 2, T_COAST = 3 };

__device__ __forceinline__ int64_t wrap(int64_t x, int n) {  // n-bit two's complement
  const uint64_t m = (uint64_t)1 << n;
  const uint64_t u = (uint64_t)x & (m - 1);
  return u >= (m >> 1) ? (int64_t)u - (int64_t)m : (int64_t)u;
}
__device__ __forceinline__ int64_t resize_s(int64_t x, int n) {  // numeric_std RESIZE(signed) shrink
  const int64_t low = x & (((int64_t)1 << (n - 1)) - 1);
  return x < 0 ? low - ((int64_t)1 << (n - 1)) : low;
}
__device__ __forceinline__ int64_t floor_shr8(int64_t x) { return x >= 0 ? x >> 8 : -((-x + 255) >> 8); }
__device__ __forceinline__ int64_t abs64(int64_t x) { return x < 0 ? -x : x; }

template <bool RTL> __device__ __forceinline__ int64_t w(int64_t x, int n) { return RTL ? wrap(x, n) : x; }
template <bool RTL> __device__ __forceinline__ int64_t rs(int64_t x, int n) { return RTL ? resize_s(x, n) : x; }
template <bool RTL> __device__ __forceinline__ uint32_t u(uint64_t x, int n) {
  return RTL ? (uint32_t)(x & ((1ull << n) - 1)) : (uint32_t)x;
}

// value of lane `src` (wave-uniform) in every lane
__device__ __forceinline__ uint32_t bcast(uint32_t v, uint32_t src) {
  return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)src);
}
__device__ __forceinline__ int64_t bcast64(int64_t v, uint32_t src) {
  const uint32_t lo = bcast((uint32_t)(uint64_t)v, src), hi = bcast((uint32_t)((uint64_t)v >> 32), src);
  return (int64_t)(((uint64_t)hi << 32) | lo);
}
__device__ __forceinline__ int64_t shfl64(int64_t v, uint32_t src) {
  const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)(uint64_t)v, (int)src, 64);
  const uint32_t hi = (uint32_t)__shfl((int)(uint32_t)((uint64_t)v >> 32), (int)src, 64);
  return (int64_t)(((uint64_t)hi << 32) | lo);
}
__device__ __forceinline__ uint64_t below(uint32_t lane) { return (1ull << lane) - 1ull; }
// position of the k-th (0-based) set bit of mask; k < popcount(mask)
__device__ __forceinline__ uint32_t kth_bit(uint64_t mask, uint32_t k) {
  uint32_t pos = 0;
#pragma unroll
  for (uint32_t wd = 32; wd; wd >>= 1) {
    const uint32_t c = (uint32_t)__popcll((mask >> pos) & ((1ull << wd) - 1ull));
    if (k >= c) {
      k -= c;
      pos += wd;
    }
  }
  return pos;
}

// Build-time alternatives of k_tws_track, for measurement only (tools/tws_dev_variants.sh builds one
// library per alternative; the shipped library uses the defaults, DESIGN.md 4e has the figures).
#ifndef FMCW_TWS_WAVEMIN
#define FMCW_TWS_WAVEMIN 1    // 0: intended-mode association by a scalar walk of the candidate ballot
#endif
#ifndef FMCW_TWS_WAVES
#define FMCW_TWS_WAVES 1      // waves (streams) per workgroup
#endif
#ifndef FMCW_TWS_PREFETCH
#define FMCW_TWS_PREFETCH 1   // 0: a scan's records are loaded when the scan begins
#endif
constexpr uint32_t kTrackWaves = FMCW_TWS_WAVES;

// minimum over the wave's 64 lanes, in every lane: the DPP row shifts and row broadcasts of a gfx9
// reduction (identity for lanes a step does not reach), the result read from lane 63
__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) {
  const int id = -1;   // 0xFFFFFFFF
#define FMCW_TWS_DPP_MIN(ctrl, rows) \
  v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(id, (int)v, ctrl, rows, 0xf, false))
  FMCW_TWS_DPP_MIN(0x111, 0xf);   // row_shr:1
  FMCW_TWS_DPP_MIN(0x112, 0xf);   // row_shr:2
  FMCW_TWS_DPP_MIN(0x114, 0xf);   // row_shr:4
  FMCW_TWS_DPP_MIN(0x118, 0xf);   // row_shr:8: lane 15 of a row holds the row's minimum
  FMCW_TWS_DPP_MIN(0x142, 0xa);   // row_bcast:15 into rows 1 and 3
  FMCW_TWS_DPP_MIN(0x143, 0xc);   // row_bcast:31 into rows 2 and 3
#undef FMCW_TWS_DPP_MIN
  return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}

__global__ void __launch_bounds__(256) k_tws_reset(uint32_t* __restrict__ state, uint32_t n_streams) {
  const size_t total = (size_t)n_streams * kStateWords;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const uint32_t wd = (uint32_t)(i % kStateWords);
    state[i] = wd == S_BEST * 64 ? kBestDistancePowerUp : wd == S_BEST * 64 + 1 ? kBestIdxPowerUp : 0u;
  }
}

// One lane's view of a scan's detection slot, as loaded (before COLLECT's field widths).
struct RawDet {
  uint32_t cnt;   // records of the scan (wave-uniform)
  uint32_t rd;    // range | doppler << 16
  float mag;
};

// Scan [b, e) of the list: lane i's slot.  RTL mode with max_dets = 64 keeps the last record that the
// wrapping 6-bit counter sent to slot i; every other case keeps record i.
template <bool RTL>
__device__ __forceinline__ RawDet load_scan(const uint8_t* __restrict__ recs, uint32_t stride, uint32_t b, uint32_t e,
                                            uint32_t n, uint32_t max_dets, uint32_t lane) {
  e = min(e, n);   // start[] is trusted only as far as the list reaches (an unordered list breaks the
  b = min(b, e);   // precondition; it must still not index beyond the examined records)
  RawDet r;
  r.cnt = e - b;
  r.rd = 0;
  r.mag = 0.f;
  if (lane < min(r.cnt, max_dets)) {
    uint32_t j = lane;
    if (RTL && max_dets == 64) j += 64u * ((r.cnt - 1u - lane) / 64u);
    const uint32_t* p = reinterpret_cast<const uint32_t*>(recs + (size_t)(b + j) * stride);
    r.rd = p[1];
    r.mag = __uint_as_float(p[2]);
  }
  return r;
}

template <bool RTL>
__global__ void __launch_bounds__(64 * kTrackWaves) k_tws_track(const uint8_t* __restrict__ recs, uint32_t stride, uint32_t cap,
                                                  const uint32_t* __restrict__ n_recs,
                                                  const uint32_t* __restrict__ start, uint32_t n_scans,
                                                  uint32_t n_streams, fmcw_tws_config c, uint32_t* __restrict__ state,
                                                  uint32_t* __restrict__ tracks, size_t track_cap,
                                                  uint32_t* __restrict__ counts, uint32_t* __restrict__ status) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t found = n_recs[0];
  const uint32_t n = min(found, cap);
  const int64_t gate_r = (int64_t)c.gate_r * 4, gate_d = (int64_t)c.gate_d * 4;

  for (uint32_t s = blockIdx.x * kTrackWaves + wave; n_scans && s < n_streams; s += gridDim.x * kTrackWaves) {
    uint32_t* const st = state + (size_t)s * kStateWords;
    auto ld64 = [&](int f) { return (int64_t)(((uint64_t)st[(f + 1) * 64 + lane] << 32) | st[f * 64 + lane]); };
    int64_t rp = ld64(S_RP_LO), dp = ld64(S_DP_LO), rv = ld64(S_RV_LO), dv = ld64(S_DV_LO);
    uint32_t hit = st[S_HIT * 64 + lane], miss = st[S_MISS * 64 + lane], quality = st[S_QUALITY * 64 + lane];
    uint32_t age = st[S_AGE * 64 + lane], last_mag = st[S_LAST_MAG * 64 + lane];
    const uint32_t flags = st[S_FLAGS * 64 + lane];
    bool active = flags & 1u;
    uint32_t tstat = (flags >> 1) & 3u;
    uint32_t best_distance = st[S_BEST * 64], best_idx = st[S_BEST * 64 + 1];   // wave-uniform

    // two scans of start words and one scan of records in flight ahead of the scan being worked on
#if FMCW_TWS_PREFETCH
    uint32_t b1 = start[s], e1 = start[s + 1];   // scan 0
    RawDet nxt = load_scan<RTL>(recs, stride, b1, e1, n, c.max_dets, lane);
    if (n_scans > 1) {
      b1 = start[(size_t)n_streams + s];
      e1 = start[(size_t)n_streams + s + 1];
    }
#endif

    for (uint32_t scan = 0; scan < n_scans; ++scan) {
      const size_t m = (size_t)scan * n_streams + s;
#if FMCW_TWS_PREFETCH
      const RawDet cur = nxt;
      if (scan + 1 < n_scans) nxt = load_scan<RTL>(recs, stride, b1, e1, n, c.max_dets, lane);
      if (scan + 2 < n_scans) {
        b1 = start[m + 2 * (size_t)n_streams];
        e1 = start[m + 2 * (size_t)n_streams + 1];
      }
#else
      const RawDet cur = load_scan<RTL>(recs, stride, start[m], start[m + 1], n, c.max_dets, lane);
#endif

      // ST_COLLECT
      const uint32_t kept = min(cur.cnt, c.max_dets);
      const uint32_t det_count = (RTL && c.max_dets == 64) ? (cur.cnt & 63u) : kept;
      const bool valid = lane < kept;
      const float mf = cur.mag;
      const uint64_t mi = mf <= 0.f ? 0ull : mf >= 4.0e9f ? 0xFFFFFFFFull : (uint64_t)(uint32_t)(mf + 0.5f);
      const int64_t er = (int64_t)u<RTL>(cur.rd & 0xffffu, 10), ed = (int64_t)u<RTL>(cur.rd >> 16, 7);
      const uint32_t emag = u<RTL>(mi, 17);
      bool assoc = false;
      // the measured position as ASSOCIATE's distance reads it (unsigned in the RTL, :165-168)
      const int64_t ar = RTL ? ((er << 2) & 0xFFF) : 4 * er, ad = RTL ? ((ed << 2) & 0x1FF) : 4 * ed;

      // ST_PREDICT
      if (active) {
        rp = w<RTL>(rp + rv, 12);
        dp = w<RTL>(dp + dv, 9);
        age = u<RTL>((uint64_t)age + 1, 8);
      }

      // ST_ASSOCIATE, track by track in slot order
      bool my_hit = false;
      uint32_t my_bi = 0;
      for (uint64_t am = __ballot(active); am; am &= am - 1) {
        const uint32_t t = (uint32_t)__builtin_ctzll(am);
        const int64_t trp = bcast64(rp, t), tdp = bcast64(dp, t);
        const int64_t dr = abs64(trp - ar), dd = abs64(tdp - ad);
        const bool gated = valid && !assoc && dr < gate_r && dd < gate_d;
        bool h = false;
        uint32_t bi = 0;
        if (RTL) {
          const uint32_t dist = (uint32_t)((dr + dd) & 0xFFFF);
          const uint64_t q = __ballot(gated && dist < best_distance);   // best_distance: the previous track's
          uint32_t bd = 0xFFFF;
          bi = 63;
          if (q) {
            bi = 63u - (uint32_t)__builtin_clzll(q);   // the last qualifying detection wins
            bd = bcast(dist, bi);
          }
          best_distance = bd;
          best_idx = bi;
          h = bi < c.max_dets && bd < 0xFFFF;
        } else if (FMCW_TWS_WAVEMIN) {
          // one wave-minimum over dist * 64 + lane (dist < 2 * 4 * 4096): 7 cross-lane steps per track
          // whatever the gates hold
          const uint32_t key = wave_min_u32(gated ? ((uint32_t)(dr + dd) << 6) | lane : 0xFFFFFFFFu);
          h = key != 0xFFFFFFFFu;
          bi = key & 63u;
        } else {
          // The measured alternative: a walk of the candidate ballot, a v_readlane and a scalar compare
          // per candidate.  Equal to the wave-minimum within 1 % at the default gates, 10 times slower
          // with every detection in every gate (up to 64 + 63 + ... + 1 = 2080 candidates per scan
          // against a fixed 7 steps per track); DESIGN.md 4e.
          const uint32_t dist = (uint32_t)(dr + dd);   // < 2 * 4 * 4096 where gated
          uint64_t q = __ballot(gated);
          if (q) {
            h = true;
            bi = (uint32_t)__builtin_ctzll(q);
            uint32_t bd = bcast(dist, bi);
            for (q &= q - 1; q; q &= q - 1) {
              const uint32_t j = (uint32_t)__builtin_ctzll(q);
              const uint32_t dj = bcast(dist, j);
              if (dj < bd) {   // strict: the lowest index wins a tie
                bd = dj;
                bi = j;
              }
            }
          }
        }
        if (h && lane == bi) assoc = true;
        if (lane == t) {
          my_hit = h;
          my_bi = bi;
        }
      }

      // ST_UPDATE, every associated track at once (an update touches its own track only)
      {
        const int64_t hr = shfl64(er, my_bi), hd = shfl64(ed, my_bi);
        const uint32_t hmag = (uint32_t)__shfl((int)emag, (int)my_bi, 64);
        if (active) {
          if (my_hit) {
            const int64_t ir = w<RTL>(w<RTL>(4 * hr, 12) - rp, 12);
            const int64_t id = w<RTL>(w<RTL>(4 * hd, 9) - dp, 9);
            const uint32_t old_hit = hit;
            const uint32_t old_status = tstat;
            rp = w<RTL>(rp + rs<RTL>(floor_shr8(ir * (int64_t)c.alpha_q8), 12), 12);
            dp = w<RTL>(dp + rs<RTL>(floor_shr8(id * (int64_t)c.alpha_q8), 9), 9);
            rv = w<RTL>(rv + rs<RTL>(floor_shr8(ir * (int64_t)c.beta_q8), 10), 10);
            dv = w<RTL>(dv + rs<RTL>(floor_shr8(id * (int64_t)c.beta_q8), 8), 8);
            hit = u<RTL>((uint64_t)old_hit + 1, 4);
            miss = 0;
            last_mag = hmag;
            if (old_status == T_TENT && old_hit >= c.init_hits) tstat = T_FIRM;
            else if (old_status == T_COAST) tstat = T_FIRM;
            if (quality < 15) ++quality;
          } else {
            const uint32_t old_miss = miss;
            miss = u<RTL>((uint64_t)old_miss + 1, 4);
            if (tstat == T_FIRM) tstat = T_COAST;
            if (old_miss >= c.coast_max) {
              active = false;
              tstat = T_FREE;
            }
            if (quality > 0) --quality;
          }
        }
      }

      // ST_INITIATE: the k-th unclaimed detection into the k-th free slot
      {
        const uint32_t n_init = (RTL && det_count == 0) ? 1u : det_count;
        const uint64_t dmask = __ballot(lane < n_init && valid && !assoc);
        const bool is_free = !active && lane < c.max_tracks;
        const uint64_t fmask = __ballot(is_free);
        const uint32_t k = (uint32_t)__popcll(fmask & below(lane));
        const bool take = is_free && k < (uint32_t)__popcll(dmask);
        const uint32_t src = take ? kth_bit(dmask, k) : lane;
        const int64_t nr = shfl64(er, src), nd = shfl64(ed, src);
        const uint32_t nmag = (uint32_t)__shfl((int)emag, (int)src, 64);
        if (take) {
          active = true;
          tstat = T_TENT;
          rp = w<RTL>(4 * nr, 12);
          dp = w<RTL>(4 * nd, 9);
          rv = 0;
          dv = 0;
          hit = 1;
          miss = 0;
          quality = 1;
          age = 0;
          last_mag = nmag;
        }
      }

      // ST_MAINTAIN + ST_OUTPUT
      {
        const bool rep = active && (tstat == T_FIRM || tstat == T_COAST);
        const uint64_t omask = __ballot(rep);
        const uint64_t amask = __ballot(active);
        const uint32_t j = (uint32_t)__popcll(omask & below(lane));
        if (rep && (size_t)j < track_cap) {
          uint32_t* o = tracks + (m * track_cap + j) * 7;   // fmcw_track: 28 bytes
          o[0] = lane | (tstat << 16) | (quality << 24);      // id u16, status u8, quality u8
          o[1] = (uint32_t)(int32_t)rp;
          o[2] = (uint32_t)(int32_t)dp;
          o[3] = (uint32_t)(int32_t)rv;
          o[4] = (uint32_t)(int32_t)dv;
          o[5] = last_mag;
          o[6] = age;
        }
        if (lane == 0) {
          counts[2 * m] = (uint32_t)__popcll(omask);
          counts[2 * m + 1] = (uint32_t)__popcll(amask);
        }
      }
    }

    auto st64 = [&](int f, int64_t v) {
      st[f * 64 + lane] = (uint32_t)(uint64_t)v;
      st[(f + 1) * 64 + lane] = (uint32_t)((uint64_t)v >> 32);
    };
    st64(S_RP_LO, rp);
    st64(S_DP_LO, dp);
    st64(S_RV_LO, rv);
    st64(S_DV_LO, dv);
    st[S_HIT * 64 + lane] = hit;
    st[S_MISS * 64 + lane] = miss;
    st[S_QUALITY * 64 + lane] = quality;
    st[S_AGE * 64 + lane] = age;
    st[S_LAST_MAG * 64 + lane] = last_mag;
    st[S_FLAGS * 64 + lane] = (active ? 1u : 0u) | (tstat << 1);
    if (lane == 0) st[S_BEST * 64] = best_distance;
    if (lane == 1) st[S_BEST * 64 + 1] = best_idx;
  }

  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const uint32_t first_out = min(start[(size_t)n_scans * n_streams], n);   // the first record at or past frame G
    status[0] = found - n;
    status[1] = n - first_out;
  }
}

}  // namespace fmcw_twsd
