// cmap_kernel.hpp -- k_cmap / k_cmap_scan / k_cmap_state: the clutter map of include/fmcw.h "Clutter
// map", a count pass, a scan and an emit pass over state that stays on the device between calls.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "det_sink.hpp"
#include "fft_device.hpp"

namespace fmcw {

// --------------------------------------------------------------------------------------
// Geometry.  A tile is a strip of `rows` = min(8192 / n_doppler, n_range) whole range rows of one
// stream's plane; a unit is (stream, tile).  Persistent workgroups of 256 threads stride over the
// units, and a unit runs all of the call's scans of its stream for its tile, so the launch count does
// not depend on n_frames.  The per-(frame, tile) counts are numbered frame-major, tiles in range order,
// so the tiles' runs, each in (range, doppler) order, concatenate to the ordered list.
//
// The workgroup keeps c of the tile's rows plus Sr halo rows on each side in LDS, (rows + 2 Sr) x
// n_doppler floats, flat; "step" i, thread tid owns the 4 cells at e = 4 (256 i + tid) of that array
// (ascending e is list order).  At most kCmSteps = 16 steps (8192 cells plus 8 halo rows of 1024); the
// step loops are fully unrolled under the uniform test i < steps, so the scan's map cells stay in
// registers (16 float4) between the test and the update.  Per scan:
//   (a) one 16-byte load of the map per step: the tile's rows and the halo rows, clamped (nonneg);
//   (b) if the stream's age has reached warmup: for the owned rows, M over the (2 Sr + 1)(2 Sd + 1)
//       neighbourhood from LDS (rows outside the plane skipped, Doppler wrapped), T and the decision;
//   (c) after a barrier (every read of the old state is done): c' of every row held, halo rows
//       included, whose recurrence needs nothing but the cell's own c and x; then a barrier.
// The count pass sums the decisions per (frame, tile).  The emit pass keeps the 4 decision bits per step
// (64 bits per thread), ranks them with a wave scan per step and the waves' totals through LDS, then
// recomputes T for the flagged cells only and stores the records below det_cap.  It ends a unit by
// storing the owned rows of c to the other copy of the planes: a neighbour may still be reading its
// halo from this one.
//
// The ages and the index of the current copy live in device words (`ctl`), read here and advanced by
// k_cmap_scan between the passes, so that a captured call advances the state at every replay:
//   ctl[0] current copy, ctl[1] the copy the emit pass reads (k_cmap_scan's snapshot of ctl[0]),
//   ctl[2 .. 2+B) ages, ctl[2+B .. 2+2B) the ages the emit pass uses (snapshot).
// --------------------------------------------------------------------------------------
constexpr int kCmNT = 256;            // threads per workgroup
constexpr int kCmTileCells = 8192;    // owned cells per tile
constexpr int kCmSteps = 16;          // steps of 1024 cells at most: tile + halo at n_doppler 1024, Sr 4
constexpr int kCmMaxSpread = 4;

struct CmapArgs {
  int ns, lg_nd;            // range rows; log2(n_doppler)
  int n_streams;
  int sr;                   // spread_range (spread_doppler is a template argument)
  int rows;                 // owned range rows per tile
  int tiles_per_plane;
  float gain, alpha, floor, clip;
  uint32_t warmup;
};

__host__ __device__ inline size_t cmap_lds_floats(int nd, int rows, int sr) { return (size_t)(rows + 2 * sr) * (size_t)nd; }

// m[c] = max(m[c], row[(d0 + c + dd) & mask]) for dd = -SD .. SD, c = 0 .. 3: the 4 + 2 SD cells once
template <int SD>
__device__ __forceinline__ void cm_row_max4(const float* row, int d0, int mask, float m[4]) {
  float v[4 + 2 * SD];
  const float4 mid = *reinterpret_cast<const float4*>(row + d0);
  v[SD] = mid.x; v[SD + 1] = mid.y; v[SD + 2] = mid.z; v[SD + 3] = mid.w;
#pragma unroll
  for (int k = 0; k < SD; ++k) {
    v[k] = row[(d0 - SD + k) & mask];
    v[SD + 4 + k] = row[(d0 + 4 + k) & mask];
  }
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int dd = 0; dd <= 2 * SD; ++dd) m[c] = fmaxf(m[c], v[c + dd]);
}

// T of the 4 cells at local row lr (global row r), columns d0 .. d0+3, from the state in LDS
template <int SD>
__device__ __forceinline__ void cm_thresh4(const float* c_lds, const CmapArgs& g, int lr, int r, int d0, float t[4]) {
  const int nd = 1 << g.lg_nd, mask = nd - 1;
  float m[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
  const int lo = max(-g.sr, -r), hi = min(g.sr, g.ns - 1 - r);
  for (int dr = lo; dr <= hi; ++dr) cm_row_max4<SD>(c_lds + (size_t)(lr + dr) * nd, d0, mask, m);
#pragma unroll
  for (int c = 0; c < 4; ++c) t[c] = fmaxf(__fmul_rn(g.alpha, m[c]), g.floor);
}

// c' of one cell: each operation rounded on its own
__device__ __forceinline__ float cm_update(float c, float x, const CmapArgs& g) {
  const float u = g.clip == 0.f ? x : fminf(x, fmaxf(__fmul_rn(g.clip, c), g.floor));
  const float t = __fsub_rn(u, c);
  const float p = __fmul_rn(g.gain, t);
  return __fadd_rn(c, p);
}

// v, in a form the optimiser cannot see through
__device__ __forceinline__ int cm_opaque(int v) {
  asm volatile("" : "+v"(v));
  return v;
}

template <bool EMIT, int SD>
__global__ void __launch_bounds__(kCmNT, 2)
k_cmap(const float* __restrict__ map, float* __restrict__ planes, const uint32_t* __restrict__ ctl, CmapArgs g,
       int n_scans, uint32_t* __restrict__ counts, const uint32_t* __restrict__ offs, fmcw_det* __restrict__ dets,
       uint32_t det_cap) {
  extern __shared__ __attribute__((aligned(16))) float cm_lds[];
  __shared__ __attribute__((aligned(16))) int s_tot[kCmSteps][kCmNT / 64];   // emit: the waves' detections per step
  __shared__ int s_wave[kCmNT / 64];                                         // count: the waves' detections of a scan
  const int nd = 1 << g.lg_nd, mask = nd - 1;
  const int rt = g.rows + 2 * g.sr;                 // rows held
  const int n_held = rt << g.lg_nd;                 // cells held
  const int steps = (n_held + 4 * kCmNT - 1) / (4 * kCmNT);
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const size_t cells = (size_t)g.ns << g.lg_nd;
  const uint32_t cur = ctl[EMIT ? 1 : 0] & 1u;
  const int n_units = g.n_streams * g.tiles_per_plane;

  for (int unit = blockIdx.x; unit < n_units; unit += gridDim.x) {
    const int b = unit / g.tiles_per_plane;
    const int ts = unit - b * g.tiles_per_plane;
    const int row_lo = ts * g.rows - g.sr;          // the plane's row of local row 0
    const uint32_t a0 = ctl[2 + (EMIT ? g.n_streams : 0) + b];
    const float* const pin = planes + ((size_t)cur * g.n_streams + b) * cells;

    // step i of thread t: its first cell, its local row, whether the plane has that row, whether the tile owns it.
    // Each phase of a scan passes its own opaque copy of tid (cm_opaque), so that the 16 unrolled steps'
    // indices and addresses are formed where they are used: hoisted out of the scan loop and kept from
    // phase to phase they take more registers than two resident workgroups per CU leave.
    auto where = [&](int i, int t, int& e, int& lr, int& r, int& d0, bool& held, bool& own) {
      e = 4 * (i * kCmNT + t);
      lr = e >> g.lg_nd;
      d0 = e & mask;
      r = row_lo + lr;
      held = e < n_held && r >= 0 && r < g.ns;
      own = held && lr >= g.sr && lr < g.sr + g.rows;
    };

    __syncthreads();   // the previous unit's last reads of the LDS
#pragma unroll
    for (int i = 0; i < kCmSteps; ++i) {
      if (i < steps) {
        int e, lr, r, d0; bool held, own;
        where(i, tid, e, lr, r, d0, held, own);
        if (held) *reinterpret_cast<float4*>(cm_lds + e) = ld_f4<false>(pin + (size_t)r * nd + d0);
      }
    }
    __syncthreads();

    for (int k = 0; k < n_scans; ++k) {
      const uint32_t f = (uint32_t)k * (uint32_t)g.n_streams + (uint32_t)b;
      const uint32_t a = a0 > 0xffffffffu - (uint32_t)k ? 0xffffffffu : a0 + (uint32_t)k;
      const float* const fmap = map + (size_t)f * cells;
      const size_t tile = (size_t)f * g.tiles_per_plane + ts;
      const int ta = cm_opaque(tid), tb = cm_opaque(tid), tb2 = cm_opaque(tid), tc = cm_opaque(tid);
      // (a)
      float4 x[kCmSteps];
#pragma unroll
      for (int i = 0; i < kCmSteps; ++i) {
        x[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (i < steps) {
          int e, lr, r, d0; bool held, own;
          where(i, ta, e, lr, r, d0, held, own);
          if (held) x[i] = nonneg4(ld_f4<EMIT>(fmap + (size_t)r * nd + d0));
        }
      }
      // (b)
      const bool test = a >= g.warmup;
      if (test) {
        uint64_t flags = 0;
        int mine = 0;
#pragma unroll
        for (int i = 0; i < kCmSteps; ++i) {
          if (i < steps) {
            int e, lr, r, d0; bool held, own;
            where(i, tb, e, lr, r, d0, held, own);
            uint32_t fl = 0;
            if (own) {
              float t[4];
              cm_thresh4<SD>(cm_lds, g, lr, r, d0, t);
              fl = (x[i].x > t[0] ? 1u : 0u) | (x[i].y > t[1] ? 2u : 0u) | (x[i].z > t[2] ? 4u : 0u) |
                   (x[i].w > t[3] ? 8u : 0u);
            }
            if constexpr (EMIT) {
              flags |= (uint64_t)fl << (4 * i);
              int total;
              wave_excl_scan(__popc(fl), total);
              if (lane == 0) s_tot[i][wv] = total;
            } else {
              mine += __popc(fl);
            }
          }
        }
        if constexpr (EMIT) {
          __syncthreads();
          uint32_t run = offs[tile];   // records of the list before the current step (uniform)
#pragma unroll
          for (int i = 0; i < kCmSteps; ++i) {
            if (i < steps) {
              const int4 tw = *reinterpret_cast<const int4*>(s_tot[i]);
              const int step_total = tw.x + tw.y + tw.z + tw.w;
              if (step_total) {
                const uint32_t fl = (uint32_t)(flags >> (4 * i)) & 15u;
                int total;
                uint32_t idx = run + (uint32_t)((wv > 0 ? tw.x : 0) + (wv > 1 ? tw.y : 0) + (wv > 2 ? tw.z : 0)) +
                               (uint32_t)wave_excl_scan(__popc(fl), total);
                if (fl) {
                  int e, lr, r, d0; bool held, own;
                  where(i, tb2, e, lr, r, d0, held, own);
                  float t[4];
                  cm_thresh4<SD>(cm_lds, g, lr, r, d0, t);
                  const float m[4] = {x[i].x, x[i].y, x[i].z, x[i].w};
#pragma unroll
                  for (int c = 0; c < 4; ++c) {
                    if (fl >> c & 1u) {
                      if (idx < det_cap) {
                        const fmcw_u4v rec = {f, (uint32_t)r | (uint32_t)(d0 + c) << 16, __float_as_uint(m[c]),
                                              __float_as_uint(t[c])};
                        *reinterpret_cast<fmcw_u4v*>(dets + idx) = rec;
                      }
                      ++idx;
                    }
                  }
                }
                run += (uint32_t)step_total;
              }
            }
          }
        } else {
          int total;
          wave_excl_scan(mine, total);
          if (lane == 0) s_wave[wv] = total;
        }
      }
      __syncthreads();   // every read of the old state is done (and s_wave is complete)
      if constexpr (!EMIT) {
        if (tid == 0) counts[tile] = test ? (uint32_t)(s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3]) : 0u;
      }
      // (c)
#pragma unroll
      for (int i = 0; i < kCmSteps; ++i) {
        if (i < steps) {
          int e, lr, r, d0; bool held, own;
          where(i, tc, e, lr, r, d0, held, own);
          if (held) {
            float4 c = x[i];
            if (a != 0) {
              const float4 o = *reinterpret_cast<const float4*>(cm_lds + e);
              c = make_float4(cm_update(o.x, x[i].x, g), cm_update(o.y, x[i].y, g), cm_update(o.z, x[i].z, g),
                              cm_update(o.w, x[i].w, g));
            }
            *reinterpret_cast<float4*>(cm_lds + e) = c;
          }
        }
      }
      __syncthreads();
    }

    if constexpr (EMIT) {
      float* const pout = planes + ((size_t)(cur ^ 1u) * g.n_streams + b) * cells;
#pragma unroll
      for (int i = 0; i < kCmSteps; ++i) {
        if (i < steps) {
          int e, lr, r, d0; bool held, own;
          where(i, tid, e, lr, r, d0, held, own);
          if (own) st_f4<false>(pout + (size_t)r * nd + d0, *reinterpret_cast<const float4*>(cm_lds + e));
        }
      }
    }
  }
}

// One workgroup: offs[i] = counts[0] + .. + counts[i-1]; status = {the sum, 0, 0, 0}.  Then, with
// n_scans > 0, the state words move on: the emit pass's snapshots (the copy it reads, the ages it
// starts from), the other copy becomes the current one and every age grows by n_scans, saturating.
// With n_tiles == 0 it writes the four words only.
constexpr int kCmScanNT = 1024;
__global__ void __launch_bounds__(kCmScanNT)
k_cmap_scan(const uint32_t* __restrict__ counts, uint32_t* __restrict__ offs, int n_tiles, uint32_t* __restrict__ status,
            uint32_t* __restrict__ ctl, int n_streams, uint32_t n_scans) {
  const uint32_t sum = tile_offsets_scan<kCmScanNT>(counts, offs, n_tiles);   // a tile has at most 8192 cells
  if (threadIdx.x < FMCW_STATUS_WORDS) status[threadIdx.x] = threadIdx.x == 0 ? sum : 0u;
  if (n_scans) {
    for (int b = (int)threadIdx.x; b < n_streams; b += kCmScanNT) {
      const uint32_t a = ctl[2 + b];
      ctl[2 + n_streams + b] = a;
      ctl[2 + b] = a > 0xffffffffu - n_scans ? 0xffffffffu : a + n_scans;
    }
    if (threadIdx.x == 0) {
      const uint32_t cur = ctl[0] & 1u;
      ctl[1] = cur;
      ctl[0] = cur ^ 1u;
    }
  }
}

// fmcw_cmap_get_state (SET false: current copy and ages -> user) / fmcw_cmap_set_state (SET true: user ->
// current copy and ages); either user pointer may be null.  n4 = float4 of the B planes.
template <bool SET>
__global__ void __launch_bounds__(256)
k_cmap_state(float* __restrict__ planes, uint32_t* __restrict__ ctl, float* __restrict__ user_planes,
             uint32_t* __restrict__ user_ages, int n_streams, size_t n4) {
  float4* const mine = reinterpret_cast<float4*>(planes) + (size_t)(ctl[0] & 1u) * n4;
  float4* const theirs = reinterpret_cast<float4*>(user_planes);
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  if (user_planes) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
      if constexpr (SET) mine[i] = theirs[i];
      else theirs[i] = mine[i];
    }
  }
  if (user_ages && blockIdx.x == 0) {
    for (int b = (int)threadIdx.x; b < n_streams; b += (int)blockDim.x) {
      if constexpr (SET) ctl[2 + b] = user_ages[b];
      else user_ages[b] = ctl[2 + b];
    }
  }
}

}  // namespace fmcw
