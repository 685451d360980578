// bearings_kernel.hpp -- k_bearings, k_bearings_status: the rx snapshot of a record's cell (MTI + Doppler
// window + single-bin DFT per channel), its phase slope across the channels, and the status words.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/fmcw.h"
#include "spec_rows.hpp"

namespace fmcw {

// --------------------------------------------------------------------------------------
// The reference is a single-channel core and has no such stage.  With n_rx > 1 the Doppler stage
// keeps sqrt(sum_rx |X_rx|^2) only, so the phase across the channels has to be recomputed: one
// Doppler bin of one range row per channel, n_rx * n_doppler points per record -- a single-bin DFT,
// not an FFT.
//
// One wavefront per record, 4 waves per workgroup, the waves striding over the records (a record's
// arithmetic never depends on which wave takes it, so the output is the same bytes under any grid).
// Lanes stride over the chirps, c = lane + 64 j: a wave's load of a row is 512 contiguous bytes.
// With MTI a lane loads x[c-1] and x[c-2] as well (spec_rows.hpp's mti_point) -- the same cache
// lines its neighbours just asked for; taking them from the neighbours' registers would need a
// lane-0 patch from the previous 64-chirp step for nothing measurable on a latency-bound job.  The
// twiddle exp(-2 pi i m / n_doppler) and the window come from two n_doppler-entry tables computed in
// fp64 at create; m = (d c) mod n_doppler is exact in 32 bits (d, c < 1024).  Each channel's per-lane
// partial sums are added over the wave with DPP (row_shr 1/2/4/8, row_bcast 15/31: det_sink.hpp
// wave_excl_scan's idiom on floats), and every lane then holds s_k.  P, power and the coherence
// denominator accumulate channel by channel (only s_{k-1} is kept, so n_rx is a run-time bound
// with no array), and lane 0 writes the 32-byte record as two 16-byte stores.
//
// Two launches, no atomic, no counter that outlives a call:
//   k_bearings         the records; each workgroup also writes how many of its records were out of
//                      range (every launched workgroup writes its word, 0 included)
//   k_bearings_status  one wave: the sum of those words, and the two status words
// Both are static: fmcw_bearings.hip alone launches them, and the library exports no handle of theirs.
// --------------------------------------------------------------------------------------
constexpr int kBearThreads = 256;
constexpr int kBearWaves = kBearThreads / 64;  // records a workgroup has in flight
constexpr uint32_t kBearMaxGrid = 2048;        // workgroups of k_bearings (8 per CU), the size of wg_bad

struct BearGeom {
  uint32_t n_frames, n_range, n_doppler, n_rx;
  float inv_spacing;
};

template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_addf(float x) {
  return x + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, ROW_MASK, 0xf, false));
}
// The wave's sum in every lane; the whole wave is active.  A fixed order: the result depends on
// the 64 inputs only, and it is part of the records' bits (cfar2d.hpp's wave_tree_sum and the
// __shfl_xor reductions add in other orders).
__device__ __forceinline__ float wave_sum(float x) {
  x = dpp_addf<0x111, 0xf>(x);  // row_shr:1
  x = dpp_addf<0x112, 0xf>(x);  // row_shr:2
  x = dpp_addf<0x114, 0xf>(x);  // row_shr:4
  x = dpp_addf<0x118, 0xf>(x);  // row_shr:8
  x = dpp_addf<0x142, 0xa>(x);  // row_bcast:15 -> rows 1, 3
  x = dpp_addf<0x143, 0xc>(x);  // row_bcast:31 -> rows 2, 3
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), 63));
}

// s_k of one row: sum_c w[c] y[c] tw[(d c) mod n_doppler], y the MTI canceller over the row.
template <int MTI>
__device__ __forceinline__ float2 snapshot(const float2* __restrict__ row, uint32_t nd, uint32_t d,
                                           const float2* __restrict__ tw, const float* __restrict__ win,
                                           uint32_t lane) {
  float re = 0.f, im = 0.f;
#pragma unroll 4
  for (uint32_t c = lane; c < nd; c += 64) {
    float2 y = mti_point<MTI>(row + c, c);
    const float w = win[c];
    const float2 t = tw[(d * c) & (nd - 1)];
    y.x *= w;
    y.y *= w;
    re += y.x * t.x - y.y * t.y;
    im += y.x * t.y + y.y * t.x;
  }
  return make_float2(wave_sum(re), wave_sum(im));
}

template <int MTI>
static __global__ void __launch_bounds__(kBearThreads)
k_bearings(const float2* __restrict__ spec, const uint8_t* __restrict__ recs, uint32_t stride, uint32_t cap,
           const uint32_t* __restrict__ n_recs, BearGeom g, const float2* __restrict__ tw, const float* __restrict__ win,
           fmcw_bearing* __restrict__ out, float2* __restrict__ snaps, uint32_t* __restrict__ wg_bad) {
  __shared__ uint32_t s_bad[kBearWaves];
  const uint32_t n = min(n_recs[0], cap);
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  uint32_t bad = 0;
  for (uint32_t i = blockIdx.x * kBearWaves + wave; i < n; i += gridDim.x * kBearWaves) {
    const uint32_t* h = reinterpret_cast<const uint32_t*>(recs + (size_t)i * stride);
    const uint32_t f = h[0], rd = h[1];
    const uint32_t r = rd & 0xffffu, d = rd >> 16;
    uint4* o = reinterpret_cast<uint4*>(out + i);
    if (f >= g.n_frames || r >= g.n_range || d >= g.n_doppler) {  // wave-uniform; reads no spectrum
      ++bad;
      if (lane == 0) {
        o[0] = make_uint4(0u, 0u, FMCW_BEARING_OUT_OF_RANGE, 0u);
        o[1] = make_uint4(0u, 0u, 0u, 0u);
      }
      if (snaps)
        for (uint32_t k = lane; k < g.n_rx; k += 64) snaps[(size_t)i * g.n_rx + k] = make_float2(0.f, 0.f);
      continue;
    }
    const float2* row = spec + (((size_t)f * g.n_rx) * g.n_range + r) * g.n_doppler;
    const size_t rx_step = (size_t)g.n_range * g.n_doppler;
    float p_re = 0.f, p_im = 0.f, pw = 0.f, den = 0.f, a_prev = 0.f;
    float2 s_prev = make_float2(0.f, 0.f);
    for (uint32_t k = 0; k < g.n_rx; ++k, row += rx_step) {
      const float2 s = snapshot<MTI>(row, g.n_doppler, d, tw, win, lane);
      if (snaps && lane == 0) snaps[(size_t)i * g.n_rx + k] = s;
      const float a2 = s.x * s.x + s.y * s.y;
      const float a = sqrtf(a2);
      pw += a2;
      if (k) {  // s_k conj(s_{k-1})
        p_re += s.x * s_prev.x + s.y * s_prev.y;
        p_im += s.y * s_prev.x - s.x * s_prev.y;
        den += a * a_prev;
      }
      s_prev = s;
      a_prev = a;
    }
    if (lane == 0) {
      uint32_t flags = 0;
      float nu = 0.f, coh = 0.f;
      if (g.n_rx == 1) {
        flags |= FMCW_BEARING_ONE_RX;
      } else {
        // 1 / (2 pi); fl(pi) fl(1 / 2 pi) may round above 0.5
        nu = fminf(fmaxf(atan2f(p_im, p_re) * 0.15915494309189535f, -0.5f), 0.5f);
        const float ap = hypotf(p_re, p_im);             // |P|^2 can leave the fp32 range
        coh = (den > 0.f && den <= 3.402823466e38f) ? ap / den : 0.f;
      }
      const float st = nu * g.inv_spacing;
      if (fabsf(st) > 1.f) flags |= FMCW_BEARING_NO_ANGLE;
      o[0] = make_uint4(f, rd, flags, __float_as_uint(nu));
      o[1] = make_uint4(__float_as_uint(st), __float_as_uint(sqrtf(pw)), __float_as_uint(coh), 0u);
    }
  }
  if (lane == 0) s_bad[wave] = bad;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t c = 0;
    for (int w = 0; w < kBearWaves; ++w) c += s_bad[w];
    wg_bad[blockIdx.x] = c;
  }
}

// One wave: the status words from the n_wg words k_bearings of the same call wrote.
static __global__ void __launch_bounds__(64)
k_bearings_status(uint32_t cap, const uint32_t* __restrict__ n_recs, const uint32_t* __restrict__ wg_bad, uint32_t n_wg,
                  uint32_t* __restrict__ n_out) {
  uint32_t c = 0;
  for (uint32_t j = threadIdx.x; j < n_wg; j += 64) c += wg_bad[j];
  for (int s = 32; s; s >>= 1) c += __shfl_xor(c, s, 64);
  if (threadIdx.x == 0) {
    n_out[0] = min(n_recs[0], cap);
    n_out[1] = c;
  }
}

}  // namespace fmcw
