// cfar1d.hpp -- magnitude rows in LDS, wave tiles and the 1-D OS-CFAR (K2's CFAR stage and k_cfar1d).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "det_sink.hpp"
#include "fft_device.hpp"

namespace fmcw {

// --------------------------------------------------------------------------------------
// Magnitude rows in LDS (K2, the 1-D CFAR and K3).  A row holds the NC cells plus a 16-cell
// circular halo on each side (cells -16..-1 = NC-16..NC-1, cells NC..NC+15 = 0..15), so a
// CFAR window of reach <= 16 never wraps and its addresses are a per-lane base plus
// immediates.  Every 16 cells are followed by 4 pad floats: each 16-cell block starts 16-B
// aligned (one ds_read_b128 per 4 cells) and 16 lanes reading blocks 16 cells apart touch 16
// disjoint bank quads (20 t mod 64 are distinct).
// --------------------------------------------------------------------------------------
// |X| from |X|^2: the hardware square root (v_sqrt_f32, <= 1 ulp) instead of the correctly
// rounded libm sequence (~15 VALU instructions each: denormal scaling plus two fma fix-ups).
// Magnitudes are specified to 1e-4 relative (BASELINE north_star), the CFAR is exact on
// whatever map is produced, and |X|^2 is never denormal-sensitive at these scales.  Scaling
// the input by 2 still scales the map by exactly 2 (an even exponent shift).
__device__ __forceinline__ float mag_sqrt(float p) { return __builtin_amdgcn_sqrtf(p); }
// |X|^2 with both products rounded before the sum.  Left to -ffp-contract, whether x*x + y*y
// becomes fma(x, x, y*y) depended on the surrounding code, so K2's variants and the paired
// kernel differed in the last bit of 7 % of the cells; with contraction off in this scope every
// kernel that computes a magnitude (K2, the fused and the paired kernels) rounds it identically.
__device__ __forceinline__ float cabs2(float2 X) {
#pragma clang fp contract(off)
  return X.x * X.x + X.y * X.y;
}

constexpr int MH = 16;  // halo cells per side
__host__ __device__ constexpr int midx(int d) { return (d + MH) + (((d + MH) >> 4) << 2); }
// midx(x + o) - midx(x) for x % 16 == 0 and a compile-time o >= -MH
__host__ __device__ constexpr int moff(int o) { return o + 4 * (o >= 0 ? o / 16 : -((15 - o) / 16)); }
// midx(x + o) - midx(x) for o >= 0 when x % 16 + o % 16 < 16 (cf. padoff)
__host__ __device__ constexpr int mpadoff(int o) { return o + 4 * (o / 16); }
template <int NC> constexpr int mrow_floats() { return (((NC + 2 * MH) * 5 / 4) + 3) & ~3; }
__host__ __device__ constexpr int floor4(int x) { return x >= 0 ? x & ~3 : -((-x + 3) & ~3); }

// Fill the circular halos of one magnitude row once its NC cells are written; the P lanes
// that share the row copy cells j = t, t + P, ... of the 32 halo cells.
template <int NC, int P>
__device__ __forceinline__ void fill_halo(float* row, int t) {
  for (int j = t; j < 2 * MH; j += P) {
    const int dst = j < MH ? NC + j : j - 2 * MH;
    const int src = j < MH ? j : NC + j - 2 * MH;
    row[midx(dst)] = row[midx(src)];
  }
}

// Cells [o0, o0 + 4 NV) of a row relative to a 16-cell-aligned lane base (o0 % 4 == 0), as NV
// 16-byte LDS reads.
template <int NV>
__device__ __forceinline__ void load_cells(const float* base, int o0, float (&v)[4 * NV]) {
#pragma unroll
  for (int c = 0; c < NV; ++c) {
    const float4 q = *reinterpret_cast<const float4*>(base + moff(o0 + 4 * c));
    v[4 * c] = q.x;
    v[4 * c + 1] = q.y;
    v[4 * c + 2] = q.z;
    v[4 * c + 3] = q.w;
  }
}

// --------------------------------------------------------------------------------------
// Wave tiles.  K2 and the stand-alone 1-D CFAR work on tiles of WR = 64 / P range rows x all
// NC Doppler cells of one frame (P = NC/16 lanes per row, 16 cells per lane), ONE WAVEFRONT
// per tile: a row's Doppler FFT, its magnitudes, its CFAR window and its detection list all
// live in that wave's private LDS region, so no workgroup barrier is ever needed.  The waves
// of a workgroup drift apart freely and one wave's HBM loads overlap another's FFT and CFAR
// arithmetic (a workgroup is only the unit of LDS allocation).  A tile is also the unit of
// detection ordering (DetSink tile = (frame, range rows)).
// --------------------------------------------------------------------------------------
constexpr int cmax(int a, int b) { return a > b ? a : b; }

template <int NC> struct DopplerGeom {
  static constexpr int P = NC / 16;                     // lanes per range row (16 cells each)
  static constexpr int WR = 64 / P;                     // range rows per wave tile
  // waves per workgroup (independent; a workgroup's waves take consecutive row groups of one
  // frame, so together they read WPB x WR x T x 8 B of every 1 KiB spectrum tile)
  static constexpr int WPB = 4;  // (8 at NC = 1024, one workgroup reading whole 128-B lines: 56.5 -> 65.3 us)
  static constexpr int NT = 64 * WPB;
  static constexpr int REGD = padded(NC) + 4;           // complex per range row (FFT)
  static constexpr int REGM = mrow_floats<NC>();        // floats per magnitude row
  static constexpr int LIST = WR * REGM;                // detection cell list (u32) offset
  // floats per wave region: the FFT rows, later the magnitude rows + the cell list
  static constexpr int WFL = cmax(2 * WR * REGD, LIST + WR * NC);
  static constexpr int LR = FinalRadix<NC, 16>::R;      // last pass radix (after pass 1)
  static constexpr int LG = 16 / LR;
  static_assert(WFL % 4 == 0 && REGM % 4 == 0, "16-B aligned rows and regions");
};

// exact k-th smallest of 2*REF registers: bitonic sort (compile-time indices), then the max of
// the ascending prefix r[0..rank] (a select chain `i == rank ? r[i] : out` is turned by LLVM
// into a private-array lookup, i.e. a scratch store + indexed load per detection).  On the bit
// patterns: CFAR cells are non-negative (unsigned order == value order), and integer min/max need
// none of the NaN-canonicalising v_max_f32 x, x, x that fminf/fmaxf of loaded values cost.
template <int REF, int GUARD>
__device__ __forceinline__ float ranked_of(float (&rf)[2 * REF], int rank) {
  constexpr int N = 2 * REF;
  static_assert((N & (N - 1)) == 0, "power-of-two reference count");
  uint32_t r[N];
#pragma unroll
  for (int i = 0; i < N; ++i) r[i] = __float_as_uint(rf[i]);
#pragma unroll
  for (int k = 2; k <= N; k <<= 1)
#pragma unroll
    for (int j = k >> 1; j > 0; j >>= 1)
#pragma unroll
      for (int i = 0; i < N; ++i) {
        const int l = i ^ j;
        if (l > i) {
          const uint32_t a = r[i], b = r[l];
          const bool up = (i & k) == 0;
          r[i] = up ? min(a, b) : max(a, b);
          r[l] = up ? max(a, b) : min(a, b);
        }
      }
  uint32_t out = r[0];
#pragma unroll
  for (int i = 1; i < N; ++i) out = max(out, i <= rank ? r[i] : r[0]);
  return __uint_as_float(out);
}

// 1-D OS-CFAR along Doppler (circular) over a wave tile's magnitude rows, plus ordered
// emission.  Lane (rr, t) tests the 16 consecutive cells d0 = 16 t .. d0 + 15 of row rr, so
// emission in lane order is (range, doppler) order.  detect <=> #{refs : fl(alpha*ref) >= cut}
// < n_ref - rank  <=>  #{fl(alpha*ref) < cut} > rank, which is cut > fl(alpha *
// sorted(refs)[rank]) (rtl/old/os_cfar.vhd:117-137) without a sort.  The count is mask-free
// integer arithmetic (lt_bit) so that hundreds of compares do not become SGPR masks.
// REF > 0: compile-time geometry (REF refs + GUARD guards per side) with the window in
// registers, screened (below); REF == 0: runtime geometry read from LDS.
// ONEG: need = n_ref - rank <= 4 known at compile time (the reference's rank 12 of 16), so
// one qualifying group of 4 rejects and the per-cell screen is a 4-way max (no runtime branch
// per cell, which also kept both screens' registers live).
template <int NC, int REF, int GUARD, bool ONEG = false>
__device__ __forceinline__ void cfar1d_wave(const float* mags, uint32_t* list, int rr, int t, int r0,
                                            int frame, int tile, const Cfar1DArgs& cf,
                                            const DetSink& sink) {
  constexpr int CELLS = 16;
  constexpr int RS = DopplerGeom<NC>::REGM;
  const float* mrow = mags + rr * RS;
  const int d0 = t * CELLS;
  const int nref = 2 * cf.ref;
  const int lane = (int)(threadIdx.x & 63);
  uint32_t bits = 0;
  int total = 0;  // detections of the wave tile (uniform), their cells in list[0, total)
  if constexpr (REF > 0) {
    // Screen, then count exactly where needed.  A group of 4 consecutive reference cells
    // whose minimum satisfies fl(alpha*min) >= cut has all 4 refs at or above cut/alpha
    // (fl(alpha*x) is monotone in x), so 4 * #{such groups} is a lower bound on
    // #{refs : fl(alpha*ref) >= cut}; once it reaches need = n_ref - rank the cell cannot
    // detect.  The exact count (16 compares) runs only for the survivors (below) and decides
    // exactly as the unscreened count.
    static_assert(REF % 4 == 0, "reference runs split into groups of 4");
    constexpr int H = REF + GUARD;
    static_assert(H <= MH, "the window stays inside the row halos");
    constexpr int NGS = REF / 4;               // groups of 4 per side
    constexpr int RO = REF + 2 * GUARD + 1;    // first right ref, relative to the first left ref
    // two halves of 8 cells (a 28-value window each) to keep the register peak low
    const float* lb = mrow + midx(d0);
    const int need = nref - cf.rank;
    constexpr bool one_group = ONEG;           // the reference (rank 12 of 16): any group rejects
    // The lane's whole window at once: cells d0 - H .. d0 + 15 + H, group minima g[k] =
    // min(w[k .. k+3]) over it computed once (2 mins per group), not per 8-cell half.
    {
      constexpr int WW = CELLS + 2 * H;        // 36 at the reference geometry
      constexpr int O0 = floor4(-H);
      constexpr int NV = (WW + (-H - O0) + 3) / 4;
      float vf[4 * NV];
      load_cells<NV>(lb, O0, vf);
      // group minima and maxima on the bit patterns (non-negative cells: unsigned order is the
      // float order; v_min/max_u32 need no NaN canonicalisation, v_min3/max3_u32 fold pairs)
      uint32_t v[4 * NV];
#pragma unroll
      for (int k = 0; k < 4 * NV; ++k) v[k] = __float_as_uint(vf[k]);
      uint32_t g[WW - 3];
      {
        uint32_t m2[WW - 1];
#pragma unroll
        for (int k = 0; k < WW - 1; ++k) m2[k] = min(v[-H - O0 + k], v[-H - O0 + k + 1]);
#pragma unroll
        for (int k = 0; k < WW - 3; ++k) g[k] = min(m2[k], m2[k + 2]);
      }
#pragma unroll
      for (int i = 0; i < CELLS; ++i) {
        const float cut = vf[-O0 + i];
        uint32_t sb;
        if (one_group) {
          // reject <=> alpha M >= cut for the largest group minimum M.  fma(alpha, M, -cut) < 0
          // (exact product) survives a few cells the rounded test would reject -- never the
          // reverse (alpha M >= cut exactly implies fl(alpha M) >= cut) -- and the exact count
          // below decides those, so the screen stays conservative.  Sign bit = survival.
          uint32_t M = g[i];
#pragma unroll
          for (int q = 1; q < NGS; ++q) M = max(M, g[i + 4 * q]);
#pragma unroll
          for (int q = 0; q < NGS; ++q) M = max(M, g[i + RO + 4 * q]);
          sb = __float_as_uint(__builtin_fmaf(cf.alpha, __uint_as_float(M), -cut)) >> 31;
        } else {
          const uint32_t cbits = __float_as_uint(cut);
          uint32_t nlt = 0;  // groups with alpha * min < cut
#pragma unroll
          for (int q = 0; q < NGS; ++q)
            nlt += lt_bit(__float_as_uint(cf.alpha * __uint_as_float(g[i + 4 * q])), cbits) +
                   lt_bit(__float_as_uint(cf.alpha * __uint_as_float(g[i + RO + 4 * q])), cbits);
          sb = 4 * (2 * NGS - (int)nlt) < need ? 1u : 0u;
        }
        bits |= sb << i;
      }
    }
    // Exact count for the survivors only, one survivor per lane.  About 12 of a tile's 1024
    // cells survive the screen on noise + targets, but they sit in ~8 of the 16 cell
    // indices, so counting per index for the whole wave (where any lane survived) cost 8 x 16
    // compares per lane; the ordered survivor list costs one 16-compare round per 64.
    int n_surv;
    const int sx = wave_excl_scan(__popc(bits), n_surv);
    if (n_surv != 0) {  // uniform
      {
        int o = sx;
        for (uint32_t m = bits; m; m &= m - 1, ++o) list[o] = ((uint32_t)rr << 16) | (uint32_t)(d0 + __builtin_ctz(m));
      }
      pass_sync<false>();
      for (int i0 = 0; i0 < n_surv; i0 += 64) {
        const int i = i0 + lane;
        bool det = false;
        uint32_t cell = 0;
        if (i < n_surv) {
          cell = list[i];
          const int d = (int)(cell & 0xffffu);
          const float* cp = mags + (int)(cell >> 16) * RS + midx(d);
          // midx(d + o) - midx(d) = o + 4 floor((q + o) / 16), q = (d + MH) % 16, |o| < 16
          const int q = (d + MH) & 15;
          auto ref = [&](int o) { return cp[o + 4 * ((q + o) >> 4)]; };
          const uint32_t cbits = __float_as_uint(cp[0]);
          uint32_t lt = 0;
#pragma unroll
          for (int j = 0; j < REF; ++j)
            lt += lt_bit(__float_as_uint(cf.alpha * ref(-GUARD - 1 - j)), cbits) +
                  lt_bit(__float_as_uint(cf.alpha * ref(GUARD + 1 + j)), cbits);
          det = (int)lt > cf.rank;
        }
        // in-place ordered compaction: every lane has read its entry of this round, and the
        // detections land at positions <= their survivor index
        const uint64_t bal = __ballot(det);
        const int pos = total + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32),
                                                               __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
        if (det) list[pos] = cell;
        total += (int)__popcll(bal);
      }
    }
  } else {
#pragma unroll
    for (int i = 0; i < CELLS; ++i) {
      const int d = d0 + i;
      const uint32_t c = __float_as_uint(mrow[midx(d)]);
      uint32_t lt = 0;
      for (int j = 1; j <= cf.ref; ++j) {
        lt += lt_bit(__float_as_uint(cf.alpha * mrow[midx((d - cf.guard - j) & (NC - 1))]), c);
        lt += lt_bit(__float_as_uint(cf.alpha * mrow[midx((d + cf.guard + j) & (NC - 1))]), c);
      }
      bits |= ((int)lt > cf.rank ? 1u : 0u) << i;
    }
    const int excl = wave_excl_scan(__popc(bits), total);
    int o = excl;
    for (uint32_t m = bits; m; m &= m - 1, ++o) list[o] = ((uint32_t)rr << 16) | (uint32_t)(d0 + __builtin_ctz(m));
  }
  const uint32_t base = det_reserve_wave(sink, tile, total);
  if (total == 0) return;  // uniform
  // Detections cluster (a target lights up consecutive cells of one lane), so the ranked
  // value is computed one detection per lane over the whole wave, from the ordered list of
  // detected cells (rr << 16 | d) in `list` (capacity: the tile's cells).
  pass_sync<false>();
  for (int i = lane; i < total; i += 64) {
    const uint32_t cell = list[i];
    const int rl = (int)(cell >> 16), d = (int)(cell & 0xffffu);
    const float* row = mags + rl * RS;
    float ranked = 0.f;
    if constexpr (REF > 0) {
      float r[2 * REF];
#pragma unroll
      for (int j = 0; j < REF; ++j) {
        r[j] = row[midx(d - GUARD - 1 - j)];
        r[REF + j] = row[midx(d + GUARD + 1 + j)];
      }
      ranked = ranked_of<REF, GUARD>(r, cf.rank);
    } else {
      for (int j = 0; j < nref; ++j) {
        const int oj = j < cf.ref ? -(cf.guard + 1 + j) : (cf.guard + 1 + j - cf.ref);
        const float vj = row[midx((d + oj) & (NC - 1))];
        int lt = 0, le = 0;
        for (int i2 = 0; i2 < nref; ++i2) {
          const int o2 = i2 < cf.ref ? -(cf.guard + 1 + i2) : (cf.guard + 1 + i2 - cf.ref);
          const float v2 = row[midx((d + o2) & (NC - 1))];
          lt += v2 < vj;
          le += v2 <= vj;
        }
        if (lt <= cf.rank && cf.rank < le) ranked = vj;
      }
    }
    const uint32_t slot = base + (uint32_t)i;
    if (slot < sink.cap) {
      fmcw_det dd;
      dd.frame = (uint32_t)frame;
      dd.range = (uint16_t)(r0 + rl);
      dd.doppler = (uint16_t)d;
      dd.mag = row[midx(d)];
      dd.threshold = cf.alpha * ranked;
      sink.scratch[slot] = dd;
    }
  }
}

// RTL-compat 1-D threshold of cell d (rtl/old/os_cfar.vhd:117-132): the 2 ref integer cells
// q17(.) around d (circular), the rank-th smallest by counting (lt <= rank < le picks it, ties
// included), T = (ranked * SCALING_MULT / SCALING_DIV) resized to 17 bits = mod 2^17.
template <int NC>
__device__ __forceinline__ uint32_t rtl1d_threshold(const float* mrow, int d, const Cfar1DArgs& cf) {
  const int nref = 2 * cf.ref;
  uint32_t ranked = 0;
  for (int j = 0; j < nref; ++j) {
    const int oj = j < cf.ref ? -(cf.guard + 1 + j) : (cf.guard + 1 + j - cf.ref);
    const float vj = q17(mrow[midx((d + oj) & (NC - 1))]);
    int lt = 0, le = 0;
    for (int i2 = 0; i2 < nref; ++i2) {
      const int o2 = i2 < cf.ref ? -(cf.guard + 1 + i2) : (cf.guard + 1 + i2 - cf.ref);
      const float v2 = q17(mrow[midx((d + o2) & (NC - 1))]);
      lt += v2 < vj;
      le += v2 <= vj;
    }
    if (lt <= cf.rank && cf.rank < le) ranked = (uint32_t)vj;
  }
  return (ranked * (uint32_t)cf.alpha) & kQ17Mask;
}

// 1-D OS-CFAR in RTL-compat arithmetic (FMCW_COMPAT_CFAR) over a wave tile's magnitude rows:
// detect q17(cut) > T with the wrapped 17-bit threshold, which is not monotone in the ranked
// cell, so every cell gets its exact ranked value (no screen).  Same ordered emission as
// cfar1d_wave.
template <int NC>
__device__ __forceinline__ void cfar1d_wave_rtl(const float* mags, uint32_t* list, int rr, int t, int r0,
                                                int frame, int tile, const Cfar1DArgs& cf,
                                                const DetSink& sink) {
  constexpr int RS = DopplerGeom<NC>::REGM;
  const float* mrow = mags + rr * RS;
  const int d0 = t * 16;
  const int lane = (int)(threadIdx.x & 63);
  uint32_t bits = 0;
  for (int i = 0; i < 16; ++i) {
    const int d = d0 + i;
    const uint32_t cut = (uint32_t)q17(mrow[midx(d)]);
    bits |= (cut > rtl1d_threshold<NC>(mrow, d, cf) ? 1u : 0u) << i;
  }
  int total;
  const int excl = wave_excl_scan(__popc(bits), total);
  {
    int o = excl;
    for (uint32_t m = bits; m; m &= m - 1, ++o) list[o] = ((uint32_t)rr << 16) | (uint32_t)(d0 + __builtin_ctz(m));
  }
  const uint32_t base = det_reserve_wave(sink, tile, total);
  if (total == 0) return;  // uniform
  pass_sync<false>();
  for (int i = lane; i < total; i += 64) {
    const uint32_t cell = list[i];
    const int rl = (int)(cell >> 16), d = (int)(cell & 0xffffu);
    const float* row = mags + rl * RS;
    const uint32_t slot = base + (uint32_t)i;
    if (slot < sink.cap) {
      fmcw_det dd;
      dd.frame = (uint32_t)frame;
      dd.range = (uint16_t)(r0 + rl);
      dd.doppler = (uint16_t)d;
      dd.mag = q17(row[midx(d)]);
      dd.threshold = (float)rtl1d_threshold<NC>(row, d, cf);
      sink.scratch[slot] = dd;
    }
  }
}

// Dispatch on the compile-time fast path (the reference geometry REF 8 / GUARD 2).
template <int NC>
__device__ __forceinline__ void cfar1d_dispatch(const float* mags, uint32_t* list, int rr, int t, int r0,
                                                int frame, int tile, const Cfar1DArgs& cf,
                                                const DetSink& sink) {
  if (cf.compat)
    cfar1d_wave_rtl<NC>(mags, list, rr, t, r0, frame, tile, cf, sink);
  else if (cf.ref == 8 && cf.guard == 2 && 2 * cf.ref - cf.rank <= 4)
    cfar1d_wave<NC, 8, 2, true>(mags, list, rr, t, r0, frame, tile, cf, sink);
  else if (cf.ref == 8 && cf.guard == 2)
    cfar1d_wave<NC, 8, 2>(mags, list, rr, t, r0, frame, tile, cf, sink);
  else
    cfar1d_wave<NC, 0, 0>(mags, list, rr, t, r0, frame, tile, cf, sink);
}

// Stand-alone 1-D OS-CFAR over a caller-supplied [frame][range][doppler] map (fmcw_cfar),
// on the same wave tiles as K2 (so tile ids, and the detection order, are the same).
template <int NC>
__global__ void __launch_bounds__(DopplerGeom<NC>::NT)
k_cfar1d(const float* __restrict__ map, int ns, int n_tiles, int frame0, int tile0, Cfar1DArgs cf,
         DetSink sink) {
  using Gm = DopplerGeom<NC>;
  constexpr int P = Gm::P, WR = Gm::WR, WPB = Gm::WPB, REGM = Gm::REGM;
  __shared__ __attribute__((aligned(16))) float lds[WPB * Gm::WFL];
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  float* const mags = lds + wv * Gm::WFL;
  uint32_t* const list = reinterpret_cast<uint32_t*>(mags + Gm::LIST);
  const int tiles_per_frame = ns / WR;
  const int nf = n_tiles / tiles_per_frame;
  for (int tile = blockIdx.x * WPB + wv; tile < n_tiles; tile += gridDim.x * WPB) {
    const int lane = opaque(threadIdx.x & 63);
    // frame-minor order: consecutive tiles are the same rows of consecutive frames, so the
    // rows that hold a target (more candidates, more detections) spread over all waves
    const int f = tile % nf;
    const int lt = tile / nf;                    // wave tile within the frame
    const int r0 = lt * WR;
    const float* src = map + ((size_t)f * ns + r0) * NC;
#pragma unroll
    for (int i = 0; i < WR * NC / 4 / 64; ++i) {
      const int e = 4 * (lane + 64 * i);
      const int rl = e / NC, d = e - rl * NC;
      *reinterpret_cast<float4*>(mags + rl * REGM + midx(d)) = nonneg4(*reinterpret_cast<const float4*>(src + e));
    }
    pass_sync<false>();
    fill_halo<NC, P>(mags + (lane / P) * REGM, lane % P);
    pass_sync<false>();
    cfar1d_dispatch<NC>(mags, list, lane / P, lane % P, r0, frame0 + f, tile0 + f * tiles_per_frame + lt, cf,
                        sink);
    pass_sync<false>();  // the region is reused by the next tile
  }
}

}  // namespace fmcw
