// spectrum.hpp -- what K1 and K2 share: the corner-turned range spectrum between them (layout, formats,
// S48 codec) and their status counters.
//
//  K1 k_range     window + range FFT + corner turn        (radar_core.vhd:267-327)
//  K2 k_doppler   Doppler window + FFT + |X| / NCI + map + 1-D OS-CFAR, one wave per tile
//                                                        (radar_core.vhd:340-374, os_cfar.vhd)
//  K3 k_cfar2d    2-D OS-CFAR over the magnitude map       (os_cfar_2d.vhd:83-230)
//     k_det_list (detlist.hip)           deterministic detection list (radar_core.vhd:396-418)
//
// Intermediate (corner-turned range spectrum) layout in HBM, per (frame, rx):
//     inter[rb][cb][RB][T]  complex fp32,  rb = r / RB, cb = c / T
// where T = chirps per K1 workgroup and RB = 128 / T range bins, so K1 writes whole 1 KiB
// chunks and K2 reads runs of (rows per wave) x T x 8 B; element (r, c) sits at
//     ((rb * NCB + cb) * RB + r % RB) * T + c % T.
// This is the corner turner's [range][chirp] order (corner_turner.vhd:80,
// rd_addr = range + doppler * N_RANGE) tiled so both sides stream full lines.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <stdint.h>

#include "fft_device.hpp"
#include "kernel_types.hpp"

namespace fmcw {

// Corner-turned spectrum element: complex fp32 (8 B) or, with FMCW_SPEC_F16, a half2 (4 B)
// holding X / N_range (|X| <= N max|x| would overflow fp16 for ADC-scale input; the 2^-log2 N
// scale is exact and K2 undoes it at load).
// Spectrum formats (fmcw.h fmcw_spectrum_dtype): SP_F32 float2 (8 B), SP_F16 half2 of X / N (4 B),
// S48 (6 B, below) in its quad (SP_S48, T >= 8), strided-quad (SP_S48S, T = 4) or strided-pair
// (SP_S48PS, T = 2) form; K1 and K2 are instantiated per form.  (Value 3 was round 5's first pair
// form -- adjacent chirps, each K2 lane loading the pair's element and decoding one point; the
// strided pair replaced it: config 3 23.9-24.5 k -> 24.4-24.5 k frames/s.)
constexpr int SP_F32 = 0, SP_F16 = 1, SP_S48 = 2, SP_S48S = 4, SP_S48PS = 5;
// strided S48 forms: the chirps a K1 group holds (and shares an exponent over) are the ones a K2
// lane holds, p = n_doppler / 16 apart (section 3 of DESIGN.md)
template <int SP> constexpr int s48_strided_g() { return SP == SP_S48S ? 4 : SP == SP_S48PS ? 2 : 0; }
template <int SP> struct SpecEl { using T = float2; };
template <> struct SpecEl<SP_F16> { using T = uint32_t; };
template <> struct SpecEl<SP_S48> { using T = S48; };
template <> struct SpecEl<SP_S48S> { using T = S48; };
template <> struct SpecEl<SP_S48PS> { using T = S48; };
typedef _Float16 fmcw_h2 __attribute__((ext_vector_type(2)));

// ---- S48: the corner-turned spectrum in 6 bytes per point, one exponent per chirp group --------
// The G chirps Gk .. Gk + G - 1 of one range bin (contiguous in a tile row) share one exponent
// E = max frexp exponent of their 2G components (|x| < 2^E), clamped to >= -95; each component is
// stored as q = rint(x 2^(W - 1 - E)), a W-bit two's-complement significand (clamped to
// 2^(W-1) - 1), so |x - q 2^(E - W + 1)| <= 2^(E - W): 2^-W of the group's largest component (or
// of 2^-95), where fp32 keeps 2^-24 of each.  By K1's tile width T:
//   quad (T >= 8, n_range <= 512): G = 4 adjacent chirps, W = 23, 2 exponent bits per point;
//   strided quad (T = 4, n_range = 1024): G = 4 chirps p apart (p = n_doppler / 16), W = 23;
//   strided pair (T = 2, n_range >= 2048): G = 2 chirps p apart, W = 22, 4 exponent bits per point.
// Point record (48 bits, little-endian, point q of the group at bytes 6q .. 6q + 5): bits 0 .. W-1
// re, then the 8/G bits (8/G) q .. of e8 = E + 127, then im in the top W bits.
// K1 lanes hold chirp pairs (c0, c0 + 1) of the group, c0 even; in the quad forms they exchange the
// pair maximum with the lane of the other pair (lane ^ 1).  K2: adjacent quads sit in lanes
// t .. t + 3 (P % 4 == 0), which OR their exponent pieces together (DPP); a strided group sits in
// one lane (the points t + p m it transforms), decoded from its whole element.  Measured on the
// CPU model (fp64 oracle, per-bin error on bins >= 1e-3 of the frame peak): quad <= 3.3e-5 over 48
// config-2 frames, pair 3.7e-8 at config 5 and 2.5e-8 at config 3, against 1e-4 allowed; one
// exponent per point with 20-bit significands reached 1.9e-4 at config 2.
typedef uint32_t fmcw_u3v __attribute__((ext_vector_type(3)));
template <int G>
__device__ __forceinline__ fmcw_u3v s48_pack(float2 v0, float2 v1, int q0) {
  static_assert(G == 2 || G == 4, "pair or quad");
  constexpr int W = G == 4 ? 23 : 22, PB = 8 / G;
  // the largest |component| by an integer max of the sign-cleared bits (finite values): fmaxf's
  // operand canonicalisation became a late `v_max_f32 vX, |vY|, |vY|` that hipcc (ROCm 7.2) placed
  // right after the previous element's dwordx3 store, overwriting that store's data VGPRs without
  // the 2 wait states the hazard needs -- intermittently corrupt tiles (tools/store_hazard_scan.py)
  constexpr uint32_t AB = 0x7fffffffu;
  const uint32_t mb = max(max(__float_as_uint(v0.x) & AB, __float_as_uint(v0.y) & AB),
                          max(__float_as_uint(v1.x) & AB, __float_as_uint(v1.y) & AB));
  // E from the largest |component| m raised by 2^-(W-1) relative: m (1 + 2^-(W-1)) < 2^E gives
  // m < 2^E (1 - 2^-W), so rint(|x| 2^(W-1-E)) <= 2^(W-1) - 1 and no significand needs a clamp (a
  // group within 2^-W of a power of two takes the next exponent: one bit less, still within 2^-W)
  int el = __builtin_amdgcn_frexp_expf(__uint_as_float(mb) * (1.0f + 1.0f / (1 << (W - 1))));
  if constexpr (G == 4) el = max(el, __builtin_amdgcn_mov_dpp(el, 0xB1 /* quad_perm [1,0,3,2]: lane ^ 1 */, 0xf, 0xf, false));
  const int E = max(el, -95);  // K2's scale 2^(E - 31) stays a normal float
  const uint32_t e8 = (uint32_t)(E + 127);
  // 2^(W-1-E) as a float (W-1-E in [-8, 117]: normal): one packed multiply scales re and im
  const float sc = __uint_as_float((uint32_t)(W - 1 - E + 127) << 23);
  typedef float f2v __attribute__((ext_vector_type(2)));
  const f2v s0 = f2v{v0.x, v0.y} * f2v{sc, sc}, s1 = f2v{v1.x, v1.y} * f2v{sc, sc};
  auto sig = [](float x) -> uint32_t { return (uint32_t)(int)__builtin_rintf(x); };
  const uint32_t r0 = sig(s0.x), i0 = sig(s0.y), r1 = sig(s1.x), i1 = sig(s1.y);
  constexpr uint32_t PM = (1u << PB) - 1;
  const uint32_t b0 = (e8 >> (PB * q0)) & PM, b1 = (e8 >> (PB * q0 + PB)) & PM;
  constexpr uint32_t MW = (1u << W) - 1;
  fmcw_u3v w;
  w.x = (r0 & MW) | (b0 << W) | (i0 << (W + PB));                                   // P0 bits 0-31
  w.y = ((i0 >> (32 - W - PB)) & 0xffffu) | (r1 << 16);                             // P0 32-47, P1 0-15
  w.z = ((r1 >> 16) & ((1u << (W - 16)) - 1)) | (b1 << (W - 16)) | (i1 << (W - 16 + PB));  // P1 16-47
  return w;
}
// Strided-quad form (SP_S48S): K2 lane t holds the 4 points of a quad (chirps t + 4 p k + p j,
// j = 0..3, as K1 grouped them) in one 24-byte element, loaded as two 12-byte halves w0 (points 0,
// 1) and w1 (points 2, 3): the exponent is assembled from the 4 records' 2-bit pieces in the lane,
// no exchange; record j's bits 0-31 / 16-47 are byte-aligned slices of the 6 words.
__device__ __forceinline__ void s48s_unpack4(fmcw_u3v w0, fmcw_u3v w1, float2 (&out)[4]) {
  const uint32_t lo[4] = {w0.x, __builtin_amdgcn_alignbyte(w0.z, w0.y, 2), w1.x, __builtin_amdgcn_alignbyte(w1.z, w1.y, 2)};
  const uint32_t hi[4] = {__builtin_amdgcn_alignbyte(w0.y, w0.x, 2), w0.z, __builtin_amdgcn_alignbyte(w1.y, w1.x, 2), w1.z};
  uint32_t e = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) e |= __builtin_amdgcn_ubfe(lo[j], 23, 2) << (2 * j);
  const float sc = __uint_as_float((e - 31) << 23);  // 2^(E - 31)
  typedef float f2v __attribute__((ext_vector_type(2)));
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const f2v r = f2v{(float)(int)(lo[j] << 9), (float)(int)(hi[j] & 0xfffffe00u)} * f2v{sc, sc};
    out[j] = make_float2(r.x, r.y);
  }
}
// Strided-pair form (SP_S48PS): a lane's points 2k, 2k + 1 (chirps t + 2 p k + p j) in one 12-byte
// element, both decoded in the lane
__device__ __forceinline__ void s48ps_unpack2(fmcw_u3v w, float2 (&out)[2]) {
  constexpr int W = 22;
  const uint32_t lo[2] = {w.x, __builtin_amdgcn_alignbyte(w.z, w.y, 2)};
  const uint32_t hi[2] = {__builtin_amdgcn_alignbyte(w.y, w.x, 2), w.z};
  const uint32_t e = __builtin_amdgcn_ubfe(w.x, W, 4) | (__builtin_amdgcn_ubfe(w.z, W - 16, 4) << 4);
  const float sc = __uint_as_float((e - 31) << 23);  // 2^(E - 31)
  typedef float f2v __attribute__((ext_vector_type(2)));
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const f2v r = f2v{(float)(int)(lo[j] << (32 - W)), (float)(int)(hi[j] & ~((1u << (32 - W)) - 1))} * f2v{sc, sc};
    out[j] = make_float2(r.x, r.y);
  }
}
// A 12-byte S48 store, padded: a VALU write of a wide store's data VGPRs within 2 wait states of
// the store corrupts the stored data under load, and hipcc (ROCm 7.2, gfx950) pads that hazard
// only for stores whose soffset is not an SGPR -- k_range_px's S48 tile stores (SGPR soffset) came
// out with the next element's packing writing into the previous store's data VGPRs at once, and
// the first frame of multi-group launches read back wrong under load (tools/store_hazard_scan.py
// finds such sequences in a .s).  The two wait states are placed here, fenced against scheduling.
// (k_range / k_range_sq store with soffset 0, which hipcc pads itself: they use the plain store,
// config-2 K1 74.3-74.7 against 74.6-75.2 us per launch with the fenced one.)
template <int AUX>
__device__ __forceinline__ void store_b96_padded(fmcw_u3v w, __amdgpu_buffer_rsrc_t rs, uint32_t vo, uint32_t so) {
  __builtin_amdgcn_raw_buffer_store_b96(w, rs, vo, so, AUX);
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_nop 1");
  __builtin_amdgcn_sched_barrier(0);
}
// One point from the 8 bytes loaded at its record's byte offset rounded down to 4 (odd = its point
// index is odd: the record starts at byte 2 of them); qs = (8/G) (c % G), the shift of its exponent
// piece.  Every lane of the group must call it together.  Two byte permutes give the record's bits
// 0-31 and 16-47; the significands land in the top W bits of a word (low bits zero), so
// v_cvt_f32_i32 reads q 2^(32-W) exactly and one packed multiply by 2^(E - 31) scales both.
template <int G>
__device__ __forceinline__ float2 s48_unpack(fmcw_u2v raw, uint32_t odd, uint32_t qs) {
  constexpr int W = G == 4 ? 23 : 22, PB = 8 / G;
  const uint32_t so = odd * 0x02020202u;
  const uint32_t w0 = __builtin_amdgcn_perm(raw.y, raw.x, 0x03020100u + so);  // record bits 0-31
  const uint32_t w1 = __builtin_amdgcn_perm(raw.y, raw.x, 0x05040302u + so);  // record bits 16-47
  const float re = (float)(int)(w0 << (32 - W)), im = (float)(int)(w1 & ~((1u << (32 - W)) - 1));
  int e = (int)(__builtin_amdgcn_ubfe(w0, W, PB) << qs);
  e |= __builtin_amdgcn_mov_dpp(e, 0xB1 /* lane ^ 1 */, 0xf, 0xf, false);
  if constexpr (G == 4) e |= __builtin_amdgcn_mov_dpp(e, 0x4E /* quad_perm [2,3,0,1]: lane ^ 2 */, 0xf, 0xf, false);
  const float sc = __uint_as_float((uint32_t)(e - 31) << 23);  // 2^(E - 31), E = e - 127 >= -95
  typedef float f2v __attribute__((ext_vector_type(2)));
  const f2v r = f2v{re, im} * f2v{sc, sc};
  return make_float2(r.x, r.y);
}
// The raw 8 bytes of point p (record at 6 p bytes from the S48 array's start): loaded from the
// 4-aligned byte 6 p - 2 (p & 1)
template <bool NT>
__device__ __forceinline__ fmcw_u2v ld_s48_raw(const S48* p, uint32_t odd) {
  return ld_u2<NT>(reinterpret_cast<const char*>(p) - 2 * odd);
}
__device__ __forceinline__ uint32_t pack_h2(float x, float y) {
  return __builtin_bit_cast(uint32_t, fmcw_h2{(_Float16)x, (_Float16)y});
}
template <bool NT>
__device__ __forceinline__ float2 ld_spec(const float2* p, float) { return ld_f2<NT>(p); }
template <bool NT>
__device__ __forceinline__ float2 ld_spec(const uint32_t* p, float scale) {
  uint32_t u;
  if constexpr (NT) u = __builtin_nontemporal_load(p);
  else u = *p;
  const fmcw_h2 h = __builtin_bit_cast(fmcw_h2, u);
  return make_float2((float)h[0] * scale, (float)h[1] * scale);
}

// Per-call status counters (fmcw.h: status words 2 / 3 of fmcw_enqueue): a thread's count, summed
// over its wave by shuffles, one atomic per wave that saw any event.  Called once per kernel, by
// every lane of the wave (after the grid-stride loop).
__device__ __forceinline__ void status_add(uint32_t* word, uint32_t n) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) n += (uint32_t)__shfl_xor((int)n, d, 64);
  if (word && n && (threadIdx.x & 63) == 0) atomicAdd(word, n);
}

}  // namespace fmcw
