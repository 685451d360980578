// doa_kernel.hpp -- k_doa_table, k_doa: the steering table as the scan reads it, and the angle resolver of
// include/fmcw.h ("Angle resolution"): scan, strongest grid point, cancel, scan again, RELAX, per record.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/fmcw.h"
#include "bearings_kernel.hpp"

namespace fmcw {

// --------------------------------------------------------------------------------------
// k_bearings' shape: one wavefront per record, 4 independent waves per workgroup striding over the
// records, no workgroup barrier in the record loop (a record's arithmetic never depends on which wave
// takes it, so the output is the same bytes under any grid).
//
// The table is kept transposed, At[k][g], so that lanes take consecutive grid points, g = lane + 64 m,
// m < M = n_grid / 64 <= 16: a wave's load of one channel's 64 points is 512 contiguous bytes.  The
// residual r (at most 64 complex) lives in the wave's 512 bytes of LDS; lane k also keeps r[k] in a
// register.  A scan reads r[k] by broadcast (every lane the same address) and accumulates y[m] over k in
// registers, k ascending; B[m] = |y[m]|^2 w[g] follows.  y and B stay in registers until the next scan:
// the amplitude and the parabola take them from the owning lanes (v_readlane; m is wave-uniform).  The
// kernel is instantiated for MC = 1, 2, 4, 8, 16 register slots per lane, the smallest that holds M, so
// that every index into y and B is a compile-time one and nothing goes to scratch.
//
// The argmax is two DPP reductions in det_sink.hpp wave_excl_scan's pattern (row_shr 1/2/4/8, row_bcast
// 15/31, lane 63 holds the result): the largest B, then the lowest g among the points that hold it.
// The cancellation's column A[g][:] is 64 strided 8-byte loads of At, once per stage.
//
// The sources found so far sit in lanes 0..3 of four registers (lane j: source j), written under
// lane == j and read back with v_readlane: no run-time index into an array.  At the end lane j < 4
// stores src[j] as one 16-byte word and lane 0 the 32-byte head.
//
// Two launches, no atomic, no counter that outlives a call: k_doa writes how many of each workgroup's
// records had no snapshot, k_bearings_status (bearings_kernel.hpp) sums those words into the status.
// --------------------------------------------------------------------------------------
constexpr int kDoaThreads = 256;
constexpr int kDoaWaves = kDoaThreads / 64;   // records a workgroup has in flight
constexpr uint32_t kDoaMaxGrid = 2048;        // workgroups of k_doa (8 per CU), the size of wg_bad
constexpr int kDoaMaxCh = 64;

struct DoaGeom {
  uint32_t n_ch, n_grid, k_max, relax_passes, refine;
  float min_rel;
};

// At[k][g] = A[g][k] and w[g] = 1 / sum_k |A[g][k]|^2 (fp64, stored as fp32) from A[g][k]; a row whose
// norm is 0 or not finite becomes zeros with w = 0.  One thread per grid point.  The squares of fp32
// values are exact in fp64, so the host's check (fmcw_doa.hip) sees the sum this kernel forms.
static __global__ void __launch_bounds__(64)
k_doa_table(const float2* __restrict__ a, uint32_t n_ch, uint32_t n_grid, float2* __restrict__ at, float* __restrict__ w) {
  const uint32_t g = blockIdx.x * 64 + threadIdx.x;
  if (g >= n_grid) return;
  double norm = 0.0;
  for (uint32_t k = 0; k < n_ch; ++k) {
    const float2 v = a[(size_t)g * n_ch + k];
    norm += (double)v.x * (double)v.x + (double)v.y * (double)v.y;
  }
  const bool ok = norm > 0.0 && norm <= 1.7976931348623157e308;   // false for NaN too
  w[g] = ok ? (float)(1.0 / norm) : 0.f;
  for (uint32_t k = 0; k < n_ch; ++k)
    at[(size_t)k * n_grid + g] = ok ? a[(size_t)g * n_ch + k] : make_float2(0.f, 0.f);
}

template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_maxf(float x) {   // x >= 0: the lanes DPP leaves out contribute 0
  return fmaxf(x, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, ROW_MASK, 0xf, false)));
}
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint32_t dpp_minu(uint32_t x) {
  return min(x, (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)x, CTRL, ROW_MASK, 0xf, false));
}
__device__ __forceinline__ float wave_max(float x) {   // of non-negative values; the whole wave is active
  x = dpp_maxf<0x111, 0xf>(x);
  x = dpp_maxf<0x112, 0xf>(x);
  x = dpp_maxf<0x114, 0xf>(x);
  x = dpp_maxf<0x118, 0xf>(x);
  x = dpp_maxf<0x142, 0xa>(x);
  x = dpp_maxf<0x143, 0xc>(x);
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), 63));
}
__device__ __forceinline__ uint32_t wave_min(uint32_t x) {
  x = dpp_minu<0x111, 0xf>(x);
  x = dpp_minu<0x112, 0xf>(x);
  x = dpp_minu<0x114, 0xf>(x);
  x = dpp_minu<0x118, 0xf>(x);
  x = dpp_minu<0x142, 0xa>(x);
  x = dpp_minu<0x143, 0xc>(x);
  return (uint32_t)__builtin_amdgcn_readlane((int)x, 63);
}
__device__ __forceinline__ float lane_value(float x, uint32_t lane) {   // lane is wave-uniform
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), (int)lane));
}

// One scan of the residual in `r` (the wave's LDS) and what follows from its strongest point.
template <int MC>
struct DoaScan {
  float y_re[MC], y_im[MC], b[MC];
  float b_max;      // B[g_best]
  uint32_t g_best;  // the lowest g that holds it

  // the value at grid point g (wave-uniform, < n_grid) of a per-lane array: a chain of selects over
  // compile-time slots, then the owning lane's value
  template <int Q>
  static __device__ __forceinline__ float slot(const float (&v)[MC], uint32_t m, float x) {
    if constexpr (Q < MC) return slot<Q + 1>(v, m, m == (uint32_t)Q ? v[Q] : x);
    return x;
  }
  __device__ __forceinline__ float at(const float (&v)[MC], uint32_t g) const {
    return lane_value(slot<1>(v, g >> 6, v[0]), g & 63);
  }

  __device__ __forceinline__ void run(const float2* r, const float2* __restrict__ at_tab, const float* __restrict__ w,
                                      const DoaGeom& geo, uint32_t lane) {
    const uint32_t M = geo.n_grid >> 6;
#pragma unroll
    for (int m = 0; m < MC; ++m) y_re[m] = y_im[m] = 0.f;
    const float2* col = at_tab + lane;
    for (uint32_t k = 0; k < geo.n_ch; ++k, col += geo.n_grid) {
      const float2 rk = r[k];   // one LDS address for the wave: a broadcast
#pragma unroll
      for (int m = 0; m < MC; ++m)
        if ((uint32_t)m < M) {
          const float2 a = col[64 * m];
          y_re[m] = fmaf(a.y, rk.y, fmaf(a.x, rk.x, y_re[m]));    // conj(a) r
          y_im[m] = fmaf(-a.y, rk.x, fmaf(a.x, rk.y, y_im[m]));
        }
    }
    float best = 0.f;
    uint32_t best_g = 0xffffffffu;
#pragma unroll
    for (int m = 0; m < MC; ++m) {
      b[m] = 0.f;
      if ((uint32_t)m < M) {
        const float wg = w[lane + 64 * m];
        const float p = fmaf(y_im[m], y_im[m], y_re[m] * y_re[m]);
        b[m] = (wg > 0.f && p >= 0.f) ? p * wg : 0.f;   // never NaN: some lane holds b_max
        if (b[m] > best || best_g == 0xffffffffu) {   // the lane's lowest m at its largest B
          best = b[m];
          best_g = lane + 64 * m;
        }
      }
    }
    b_max = wave_max(best);
    g_best = wave_min(best == b_max ? best_g : 0xffffffffu);
  }

  __device__ __forceinline__ float pos(const DoaGeom& geo) const {
    float off = 0.f;
    if (geo.refine && g_best > 0 && g_best + 1 < geo.n_grid) {
      const float bm = at(b, g_best - 1), bp = at(b, g_best + 1);
      const float den = bm - 2.f * b_max + bp;
      if (den < 0.f) off = 0.5f * (bm - bp) / den;
    }
    return (float)g_best + off;
  }
};

template <int MC>
static __global__ void __launch_bounds__(kDoaThreads)
k_doa(const float2* __restrict__ snaps, const uint8_t* __restrict__ cells, uint32_t stride, uint32_t cap,
      const uint32_t* __restrict__ n_recs, DoaGeom geo, const float2* __restrict__ at_tab, const float* __restrict__ w,
      fmcw_doa* __restrict__ out, float* __restrict__ spectrum, uint32_t* __restrict__ wg_bad) {
  __shared__ float2 s_r[kDoaWaves][kDoaMaxCh];
  __shared__ uint32_t s_bad[kDoaWaves];
  const uint32_t n = min(n_recs[0], cap);
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  float2* r = s_r[wave];
  const bool mine = lane < geo.n_ch;   // lane k owns channel k
  uint32_t bad = 0;
  for (uint32_t i = blockIdx.x * kDoaWaves + wave; i < n; i += gridDim.x * kDoaWaves) {
    uint32_t cell0 = 0, cell1 = 0;
    if (cells) {
      const uint32_t* h = reinterpret_cast<const uint32_t*>(cells + (size_t)i * stride);
      cell0 = h[0];
      cell1 = h[1];
    }
    float2 rk = mine ? snaps[(size_t)i * geo.n_ch + lane] : make_float2(0.f, 0.f);
    const bool finite = fabsf(rk.x) <= 3.402823466e38f && fabsf(rk.y) <= 3.402823466e38f;   // false for NaN
    const bool usable = __ballot(!finite) == 0 && __ballot(rk.x != 0.f || rk.y != 0.f) != 0;
    uint32_t flags = geo.n_ch == 1 ? FMCW_DOA_ONE_CH : 0u;
    uint32_t n_src = 0;
    float total = 0.f, residual = 0.f;
    // lane j: source j
    uint32_t src_g = 0;
    float src_pos = 0.f, src_re = 0.f, src_im = 0.f;
    float* spec_row = spectrum ? spectrum + (size_t)i * geo.n_grid : nullptr;
    if (!usable) {
      ++bad;
      flags |= FMCW_DOA_NO_SNAPSHOT;
      if (spec_row)
        for (uint32_t g = lane; g < geo.n_grid; g += 64) spec_row[g] = 0.f;
    } else {
      total = wave_sum(fmaf(rk.y, rk.y, rk.x * rk.x));
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");   // the last record's reads of r are done
      r[lane] = rk;
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
      DoaScan<MC> sc;
      // r -= a A[g][:], in the register and in LDS
      auto cancel = [&](float a_re, float a_im, uint32_t g) __attribute__((always_inline)) {
        if (mine) {
          const float2 c = at_tab[(size_t)lane * geo.n_grid + g];
          rk.x = fmaf(a_im, c.y, fmaf(-a_re, c.x, rk.x));
          rk.y = fmaf(-a_im, c.x, fmaf(-a_re, c.y, rk.y));
        }
        r[lane] = rk;
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
      };
      // source j from the scan in sc: its grid point, position and amplitude, and the cancellation
      auto fix = [&](uint32_t j) __attribute__((always_inline)) {
        const float wg = w[sc.g_best];
        const float a_re = sc.at(sc.y_re, sc.g_best) * wg, a_im = sc.at(sc.y_im, sc.g_best) * wg;
        const float p = sc.pos(geo);
        if (lane == j) {
          src_g = sc.g_best;
          src_pos = p;
          src_re = a_re;
          src_im = a_im;
        }
        cancel(a_re, a_im, sc.g_best);
      };
      float b0 = 0.f;
      for (uint32_t j = 0; j < geo.k_max; ++j) {
        sc.run(r, at_tab, w, geo, lane);
        if (j == 0) {
          b0 = sc.b_max;
          if (spec_row) {
#pragma unroll
            for (int m = 0; m < MC; ++m)
              if ((uint32_t)m < (geo.n_grid >> 6)) spec_row[lane + 64 * m] = sc.b[m];
          }
        }
        if (sc.b_max == 0.f || (j > 0 && sc.b_max < geo.min_rel * b0)) break;
        fix(j);
        n_src = j + 1;
      }
      for (uint32_t pass = 0; pass < geo.relax_passes; ++pass)
        for (uint32_t j = 0; j < n_src; ++j) {
          const uint32_t g_old = (uint32_t)__builtin_amdgcn_readlane((int)src_g, (int)j);
          cancel(-lane_value(src_re, j), -lane_value(src_im, j), g_old);   // a_j A[g_j][:] back in
          sc.run(r, at_tab, w, geo, lane);
          fix(j);
        }
      residual = wave_sum(fmaf(rk.y, rk.y, rk.x * rk.x));
    }
    uint4* o = reinterpret_cast<uint4*>(out + i);
    if (lane == 0) {
      o[0] = make_uint4(cell0, cell1, flags, n_src);
      o[1] = make_uint4(__float_as_uint(total), __float_as_uint(residual), 0u, 0u);
    }
    if (lane < FMCW_DOA_MAX_SRC)
      o[2 + lane] = lane < n_src ? make_uint4(src_g, __float_as_uint(src_pos), __float_as_uint(src_re), __float_as_uint(src_im))
                                 : make_uint4(0u, 0u, 0u, 0u);
  }
  if (lane == 0) s_bad[wave] = bad;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t c = 0;
    for (int q = 0; q < kDoaWaves; ++q) c += s_bad[q];
    wg_bad[blockIdx.x] = c;
  }
}

}  // namespace fmcw
