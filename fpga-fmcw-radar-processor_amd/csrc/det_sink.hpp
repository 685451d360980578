// det_sink.hpp -- what the CFAR kernels share: the detection sink, scans, bit-pattern compares.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernel_types.hpp"

namespace fmcw {

// Reserve a tile's range in the sink: every thread gets the same base.  `total` is uniform;
// the overflow branch (rare) needs one broadcast through LDS.
__device__ __forceinline__ uint32_t det_reserve(const DetSink& sink, int wg, int total, int* s_bcast) {
  uint32_t base = (uint32_t)wg * sink.slot_cap;
  if ((uint32_t)total > sink.slot_cap) {
    if (threadIdx.x == 0) {
      uint32_t b = sink.ovf_base + atomicAdd(sink.counter, (uint32_t)total);
      if (b + (uint32_t)total > sink.cap) atomicAdd(sink.counter + 1, b + (uint32_t)total - max(b, sink.cap));
      *s_bcast = (int)b;
    }
    __syncthreads();
    base = (uint32_t)*s_bcast;
  }
  if (threadIdx.x == 0) {
    sink.wg_base[wg] = base;
    sink.wg_count[wg] = (uint32_t)total;
  }
  return base;
}

// Exclusive scan of one int per thread over the workgroup (one barrier): wave scans by
// shuffles, each thread then adds the totals of the earlier waves.  s_wave[NT/64] must not
// be rewritten before every thread has passed (callers end the tile with a barrier).
template <int NT>
__device__ __forceinline__ int block_excl_scan1(int v, int* s_wave, int& total) {
  constexpr int NW = NT / 64;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int x = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int y = __shfl_up(x, d, 64);
    if (lane >= d) x += y;
  }
  if (lane == 63) s_wave[wv] = x;
  __syncthreads();
  int before = 0, all = 0;
#pragma unroll
  for (int i = 0; i < NW; ++i) {
    const int w = s_wave[i];
    before += i < wv ? w : 0;
    all += w;
  }
  total = all;
  return before + x - v;
}

template <int NT>
__device__ __forceinline__ int block_excl_scan(int v, int* s_wave, int& total) {
  constexpr int NW = NT / 64;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int x = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int y = __shfl_up(x, d, 64);
    if (lane >= d) x += y;
  }
  if (lane == 63) s_wave[wv] = x;
  __syncthreads();
  if (threadIdx.x == 0) {
    int acc = 0;
    for (int i = 0; i < NW; ++i) {
      const int tt = s_wave[i];
      s_wave[i] = acc;
      acc += tt;
    }
    s_wave[NW] = acc;
  }
  __syncthreads();
  total = s_wave[NW];
  const int r = s_wave[wv] + x - v;
  __syncthreads();
  return r;
}

// The scan between a detector's count pass and its emit pass, for one workgroup of NT threads:
// offs[i] = counts[0] + .. + counts[i-1] for i < n_tiles; returns the sum of all counts, in every
// thread.  Rounds of NT tiles, the running total carried from one round to the next.  counts may be
// offs (a thread reads its element before it writes it, and no other thread touches that element),
// hence no __restrict__.  A round's counts sum to less than 2^31.
template <int NT>
__device__ __forceinline__ uint32_t tile_offsets_scan(const uint32_t* counts, uint32_t* offs, int n_tiles) {
  __shared__ int s_wave[NT / 64 + 1];
  uint32_t carry = 0;
  for (int base = 0; base < n_tiles; base += NT) {
    const int i = base + (int)threadIdx.x;
    const int v = i < n_tiles ? (int)counts[i] : 0;
    int total;
    const int ex = block_excl_scan<NT>(v, s_wave, total);
    if (i < n_tiles) offs[i] = carry + (uint32_t)ex;
    carry += (uint32_t)total;
  }
  return carry;
}

// Wave-level exclusive scan; `total` = the wave's sum, uniform.  DPP adds on the VALU (GCN
// row scan: row_shr 1/2/4/8 inside each row of 16 lanes, then row_bcast:15 / row_bcast:31 carry
// the row totals), where the former __shfl_up version took six ds_bpermute round trips through
// LDS plus a lane-mask select per step (SGPR pressure).  Every caller runs it with the whole wave
// active.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ int dpp_add(int x) {
  return x + __builtin_amdgcn_update_dpp(0, x, CTRL, ROW_MASK, 0xf, false);
}
__device__ __forceinline__ int wave_excl_scan(int v, int& total) {
  int x = v;
  x = dpp_add<0x111, 0xf>(x);  // row_shr:1
  x = dpp_add<0x112, 0xf>(x);  // row_shr:2
  x = dpp_add<0x114, 0xf>(x);  // row_shr:4
  x = dpp_add<0x118, 0xf>(x);  // row_shr:8
  x = dpp_add<0x142, 0xa>(x);  // row_bcast:15 -> rows 1, 3
  x = dpp_add<0x143, 0xc>(x);  // row_bcast:31 -> rows 2, 3
  total = __builtin_amdgcn_readlane(x, 63);
  return x - v;
}

// det_reserve for a one-wave tile: its slot, or (rare) a range in the overflow region
// reserved by lane 0 and broadcast by a shuffle.  `total` is wave-uniform.
__device__ __forceinline__ uint32_t det_reserve_wave(const DetSink& sink, int tile, int total) {
  const int lane = threadIdx.x & 63;
  uint32_t base = (uint32_t)tile * sink.slot_cap;
  if ((uint32_t)total > sink.slot_cap) {
    uint32_t b = 0;
    if (lane == 0) {
      b = sink.ovf_base + atomicAdd(sink.counter, (uint32_t)total);
      if (b + (uint32_t)total > sink.cap) atomicAdd(sink.counter + 1, b + (uint32_t)total - max(b, sink.cap));
    }
    base = (uint32_t)__shfl((int)b, 0, 64);
  }
  if (lane == 0) {
    sink.wg_base[tile] = base;
    sink.wg_count[tile] = (uint32_t)total;
  }
  return base;
}

// 1 if x < y, for non-negative finite floats given as bit patterns (their unsigned order is
// the float order and |xb - yb| < 2^31).  CFAR inputs are magnitudes (>= +0), like the
// reference's unsigned magnitude stream (magnitude_calc.vhd).  No VCC / SGPR mask involved.
__device__ __forceinline__ uint32_t lt_bit(uint32_t xb, uint32_t yb) { return (xb - yb) >> 31; }

// Caller-supplied maps (fmcw_cfar) enter the CFAR as the RTL's unsigned magnitude stream:
// negative cells and -0.0 become +0 (integer max on the bit pattern: every pattern with the
// sign bit set is negative as an int32), so the bit-pattern compares above stay exact.
__device__ __forceinline__ float nonneg(float x) { return __int_as_float(max(__float_as_int(x), 0)); }
__device__ __forceinline__ float4 nonneg4(float4 v) {
  return make_float4(nonneg(v.x), nonneg(v.y), nonneg(v.z), nonneg(v.w));
}
// RTL-compat cell (FMCW_COMPAT_CFAR): the 17-bit unsigned CFAR input word (DATA_WIDTH 17,
// os_cfar.vhd:13, os_cfar_2d.vhd:11), q = min(floor(max(x, 0)), 2^17 - 1); exact in fp32.
constexpr uint32_t kQ17Mask = (1u << 17) - 1u;
__device__ __forceinline__ float q17(float x) { return fminf(floorf(nonneg(x)), (float)kQ17Mask); }
__device__ __forceinline__ float4 q17x4(float4 v) { return make_float4(q17(v.x), q17(v.y), q17(v.z), q17(v.w)); }

}  // namespace fmcw
