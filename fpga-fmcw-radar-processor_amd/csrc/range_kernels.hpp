// range_kernels.hpp -- K1: window + range FFT + corner turn (k_range, k_range_sq, k_range_px).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#include "fft_device.hpp"
#include "spectrum.hpp"

namespace fmcw {

// K1 spectrum stores at N <= 4096 are write-through (sc1): measured at config 2 (two boxes) K1
// 62.2 -> 60.5 us per 96-frame launch, 756 -> 768 k frames/s; config 3 neutral; config 5 (N = 8192)
// K1 64.9 -> 68.5 us per launch with them, so k_range_px stores write-back.  K2's map stores stay
// non-temporal write-back (write-through: K2 55.5 -> 59.5 us per launch at config 2).  Every other
// alternative measured in rounds 1-4 ("removed after measurement") is gone
// from the sources; the numbers stay in DESIGN.md and the lab builds in git history.
constexpr bool kK1WriteThrough = true;

// --------------------------------------------------------------------------------------
// Input loaders: two consecutive complex samples -> float4 (re0, im0, re1, im1).
// ADC word {Q[31:16], I[15:0]} (rtl/src/tb_radar_core.vhd:115-118) = little-endian short2(I,Q).
// fetch() issues the load and returns the raw bits; expand() converts them.  K1 prefetches the
// raw bits and expands them only when it consumes them: a conversion next to the load would
// make the prefetch wait for its data at once (fp16 / int16 input, config 5).
// --------------------------------------------------------------------------------------
// fetch1 / expand1: one complex sample per lane (k_range_sq's radix-16 first pass).
template <bool NT>
__device__ __forceinline__ uint32_t ld_u1(const void* p) {
  if constexpr (NT) return __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(p));
  else return *reinterpret_cast<const uint32_t*>(p);
}
struct LoadF32 {
  static constexpr int bytes = 8;
  using Raw = float4;
  using Raw1 = float2;
  __device__ __forceinline__ static Raw fetch(const void* base, size_t idx) {
    return ld_f4<kNtCube>(reinterpret_cast<const float2*>(base) + idx);
  }
  __device__ __forceinline__ static float4 expand(Raw r) { return r; }
  __device__ __forceinline__ static float4 load2(const void* base, size_t idx) { return fetch(base, idx); }
  __device__ __forceinline__ static Raw1 fetch1(const void* base, size_t idx) {
    return ld_f2<kNtCube>(reinterpret_cast<const float2*>(base) + idx);
  }
  __device__ __forceinline__ static float2 expand1(Raw1 r) { return r; }
  __device__ __forceinline__ static float2 expand1_scaled(Raw1 r, float s) { return make_float2(r.x * s, r.y * s); }
};
struct LoadF16 {
  static constexpr int bytes = 4;
  using Raw = fmcw_u2v;
  using Raw1 = uint32_t;
  __device__ __forceinline__ static Raw fetch(const void* base, size_t idx) {
    return ld_u2<kNtCube>(reinterpret_cast<const uint32_t*>(base) + idx);
  }
  __device__ __forceinline__ static float4 expand(Raw u) {
    typedef _Float16 h4 __attribute__((ext_vector_type(4)));
    const h4 h = __builtin_bit_cast(h4, u);
    return make_float4((float)h[0], (float)h[1], (float)h[2], (float)h[3]);
  }
  __device__ __forceinline__ static float4 load2(const void* base, size_t idx) { return expand(fetch(base, idx)); }
  __device__ __forceinline__ static Raw1 fetch1(const void* base, size_t idx) {
    return ld_u1<kNtCube>(reinterpret_cast<const uint32_t*>(base) + idx);
  }
  __device__ __forceinline__ static float2 expand1(Raw1 u) {
    typedef _Float16 h2 __attribute__((ext_vector_type(2)));
    const h2 h = __builtin_bit_cast(h2, u);
    return make_float2((float)h[0], (float)h[1]);
  }
  // (I, Q) * s: v_fma_mix_f32 converts the half and multiplies in one instruction (fma(x, s, 0) =
  // fl(x s): the fp16 -> fp32 conversion is exact)
  __device__ __forceinline__ static float2 expand1_scaled(Raw1 u, float s) {
    float re, im;
    asm("v_fma_mix_f32 %0, %1, %2, 0 op_sel_hi:[1,0,0]" : "=v"(re) : "v"(u), "v"(s));
    asm("v_fma_mix_f32 %0, %1, %2, 0 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(im) : "v"(u), "v"(s));
    return make_float2(re, im);
  }
};
struct LoadI16 {
  static constexpr int bytes = 4;
  using Raw = fmcw_u2v;
  using Raw1 = uint32_t;
  __device__ __forceinline__ static Raw fetch(const void* base, size_t idx) {
    return ld_u2<kNtCube>(reinterpret_cast<const uint32_t*>(base) + idx);
  }
  __device__ __forceinline__ static float4 expand(Raw u) {
    typedef short s4 __attribute__((ext_vector_type(4)));
    const s4 s = __builtin_bit_cast(s4, u);
    return make_float4((float)s[0], (float)s[1], (float)s[2], (float)s[3]);
  }
  __device__ __forceinline__ static float4 load2(const void* base, size_t idx) { return expand(fetch(base, idx)); }
  __device__ __forceinline__ static Raw1 fetch1(const void* base, size_t idx) {
    return ld_u1<kNtCube>(reinterpret_cast<const uint32_t*>(base) + idx);
  }
  __device__ __forceinline__ static float2 expand1(Raw1 u) {
    typedef short s2 __attribute__((ext_vector_type(2)));
    const s2 s = __builtin_bit_cast(s2, u);
    return make_float2((float)s[0], (float)s[1]);
  }
  __device__ __forceinline__ static float2 expand1_scaled(Raw1 u, float w) {
    const float2 x = expand1(u);
    return make_float2(x.x * w, x.y * w);
  }
};

// chirp q of group cb: cb T + q, or (strided S48, T = G) t + T p k + p q, the chirps of K2's lane t
// (cb = t + p k, p = nc / 16 lanes per Doppler row, lgp = log2 p), whose T points K2 then holds in one lane
template <int T, bool STRIDED>
__device__ __forceinline__ int chirp_of(int cb, int q, int lgp) {
  if constexpr (STRIDED) return (cb & ((1 << lgp) - 1)) + ((cb >> lgp) << (lgp + __builtin_ctz(T))) + (q << lgp);
  else return cb * T + q;
}

// K1 geometry per range-FFT size: T chirps per workgroup, RB = 128/T (1 KiB chunks).
template <int N> struct RangeGeom {
  static constexpr int P = N / 16;                   // threads per transform
  // Measured on MI355X (config 2, tools/ablate.py over build variants): at N = 1024, T = 4
  // (4 waves, 35 KiB LDS, 3 workgroups per CU at 141 VGPRs) beats T = 8 (8 waves, one
  // workgroup per CU) by 9 % in K1 with K2 unchanged; T = 2 is 3 % faster again in K1 but
  // halves K2's read runs (64 B) and costs more there than it saves.
  static constexpr int T = N <= 128 ? 16 : N <= 512 ? 8 : N == 1024 ? 4 : 2;
  static constexpr int NT = T * P;                   // threads per workgroup
  static constexpr int RB = 128 / T;                 // range bins per 1 KiB chunk
  static constexpr int REG = padded(N) + 4;          // LDS row (complex) per chirp
  static constexpr bool WG_SYNC = P > 64;            // transform spans several waves
};

// --------------------------------------------------------------------------------------
// K1: window + range FFT + corner turn.  One workgroup = T chirps of one (frame, rx),
// grid-stride over all chirp groups.  Each thread: 8 coalesced 16-B loads, windowing,
// radix-8 pass in registers, Stockham passes through LDS, then the tiled transposed store.
// --------------------------------------------------------------------------------------
// Q15 = RTL-compat integer range window (FMCW_WIN_Q15_RTL, int16 input): `win` then holds the
// ROM integers c[n] (exact in fp32) and each sample is windowed as sat16((x c + 2^14) >> 14)
// (window_multiplier.vhd:146-158) before it becomes fp32.
// SP = spectrum format: SP_F16 (FMCW_SPEC_F16) tiles hold half2(X / N) (8-B stores of two chirps),
// SP_S48 (FMCW_SPEC_S48) two 6-B S48 points (12-B stores; the quad form at T >= 4, pair at T = 2).
template <int N, typename LD, bool Q15 = false, int SP = SP_F32>
__global__ void __launch_bounds__(RangeGeom<N>::NT)
__attribute__((amdgpu_waves_per_eu(1)))
k_range(const void* __restrict__ cube, float2* __restrict__ inter, const float* __restrict__ win,
        const float* __restrict__ chirp_w, int nc, int n_groups, float q15_scale, uint32_t* __restrict__ status) {
  using Gm = RangeGeom<N>;
  constexpr int P = Gm::P, T = Gm::T, RB = Gm::RB, REG = Gm::REG;
  __shared__ __attribute__((aligned(16))) float2 lds[T * REG];

  const int tid = threadIdx.x;
  const int q = tid / P;  // chirp within the group
  const int t0 = tid % P;
  const int ncb = nc / T;

  // transposed-store geometry: piece i of this thread is range r0 + i*N/8, chirps c0, c0+1
  const int e0 = 2 * tid;
  const int chunk0 = e0 / (RB * T);
  const int win0 = e0 - chunk0 * (RB * T);
  const int r0 = chunk0 * RB + win0 / T;
  const int c0 = win0 % T;
  constexpr int CI = T * N / 1024;  // chunks advanced per piece
  const int rd0_off = c0 * REG + pad16(r0);

  int g = blockIdx.x;
  uint32_t n_sat = 0;     // Q15: windowed samples this thread saturated
  typename LD::Raw a[8];  // this group's samples, raw (expanded at use)
  // Doppler window of the next chirp, loaded with its samples: a vector load issued after the
  // previous iteration's eight tile stores would make the wait for it (vmcnt counts in issue
  // order) wait for those stores too.  From N = 1024 a wave holds one chirp (P >= 64), so the
  // index is wave-uniform and the load goes through the scalar cache (lgkmcnt, not vmcnt).
  auto cw_index = [](int i) { return P >= 64 ? __builtin_amdgcn_readfirstlane(i) : i; };
  constexpr int SGS = s48_strided_g<SP>();
  static_assert(SGS == 0 || SGS == T, "strided S48: one exponent group per K1 group");
  const int lgp = __builtin_ctz(nc) - 4;
  float cw_n = 1.f;
  if (g < n_groups) {
    const int fr = g / ncb;
    const int cb = g - fr * ncb;
    const size_t chirp = (size_t)fr * nc + (size_t)chirp_of<T, (SGS > 0)>(cb, q, lgp);
#pragma unroll
    for (int m = 0; m < 8; ++m) a[m] = LD::fetch(cube, chirp * N + 2 * t0 + (N / 8) * m);
    if (chirp_w) cw_n = chirp_w[cw_index(chirp_of<T, (SGS > 0)>(cb, q, lgp))];
  }
  // window coefficients for samples 2t + {0,1} + (N/8) m, held for the whole kernel (round 4:
  // re-reading them every group below N = 4096 measured 845-848 k against 856-857 k frames/s)
  constexpr bool HOLD_W = true;
  float2 wh[HOLD_W ? 8 : 1];
  if constexpr (HOLD_W) {
#pragma unroll
    for (int m = 0; m < 8; ++m) wh[m] = *reinterpret_cast<const float2*>(win + 2 * t0 + (N / 8) * m);
    // complete them here: loads still in flight at the loop header make the compiler's
    // wait there vmcnt(0), i.e. also on the previous iteration's tile stores
#pragma unroll
    for (int m = 0; m < 8; ++m) asm volatile("" ::"v"(wh[m].x), "v"(wh[m].y));
  }
  for (; g < n_groups; g += gridDim.x) {
    const int fr = g / ncb;  // frame*nrx + rx within this chunk
    const int cb = g - fr * ncb;
    const int t = opaque(t0);
    float2* buf = lds + q * REG;
    // Doppler window of this chirp folded in (K2 then skips it; FFT linearity), or 1
    const float cw = cw_n * (SP == SP_F16 ? 1.0f / N : 1.0f);

    float2 w[8];
#pragma unroll
    for (int m = 0; m < 8; ++m)
      w[m] = HOLD_W ? wh[HOLD_W ? m : 0] : *reinterpret_cast<const float2*>(win + 2 * t + (N / 8) * m);

    __syncthreads();  // previous group's transposed reads are done with lds
    float4 ax[8];
#pragma unroll
    for (int m = 0; m < 8; ++m) ax[m] = LD::expand(a[m]);
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      float2 v[8];
#pragma unroll
      for (int m = 0; m < 8; ++m) {
        if constexpr (Q15) {
          const int c = (int)(e ? w[m].y : w[m].x);
          const float xi = e ? ax[m].z : ax[m].x, xq = e ? ax[m].w : ax[m].y;
          uint32_t clip = 0;  // the sample's saturation_flag (I or Q clipped, window_multiplier.vhd:152-158)
          auto win16 = [c, &clip](float x) {
            const int y = ((int)x * c + (1 << 14)) >> 14;  // floor: arithmetic shift
            const int ys = min(max(y, -32768), 32767);
            clip |= (uint32_t)(ys != y);
            return (float)ys;
          };
          // 2^-range_shift (the IP's scaling schedule) applies after the integer window
          v[m] = make_float2(win16(xi) * (cw * q15_scale), win16(xq) * (cw * q15_scale));
          n_sat += clip;
        } else {
          const float we = (e ? w[m].y : w[m].x) * cw;
          v[m] = e ? make_float2(ax[m].z * we, ax[m].w * we) : make_float2(ax[m].x * we, ax[m].y * we);
        }
      }
      Dft<8>::run(v);
      float2* d = buf + pad16((2 * t + e) * 8);
#pragma unroll
      for (int m = 0; m < 8; ++m) d[m] = v[m];
    }
    // prefetch the next group into the (now free) input registers
    {
      const int gn = g + gridDim.x;
      if (gn < n_groups) {
        const int frn = gn / ncb;
        const int cbn = gn - frn * ncb;
        const size_t chirp = (size_t)frn * nc + (size_t)chirp_of<T, (SGS > 0)>(cbn, q, lgp);
#pragma unroll
        for (int m = 0; m < 8; ++m) a[m] = LD::fetch(cube, chirp * N + 2 * t + (N / 8) * m);
        if (chirp_w) cw_n = chirp_w[cw_index(chirp_of<T, (SGS > 0)>(cbn, q, lgp))];
      }
    }
    pass_sync<Gm::WG_SYNC>();
    stockham_from<N, 8, P, Gm::WG_SYNC>(buf, t);
    __syncthreads();

    // tiled corner turn: element (r, c) -> inter[rb][cb][RB][T]
    const float2* rd0 = lds + opaque(rd0_off);
    const size_t dbase = (size_t)fr * N * nc + ((size_t)chunk0 * ncb + cb) * (RB * T) + win0;
    float2* dst = inter + dbase;
    uint2* dst16 = reinterpret_cast<uint2*>(reinterpret_cast<uint32_t*>(inter) + dbase);
    const size_t dstep = (size_t)CI * ncb * (RB * T);
    // write-through stores (the launch's spectrum is < 4 GiB: fmcw_create caps the chunk)
    const __amdgpu_buffer_rsrc_t wrs = wt_rsrc(inter, 0xffffffffu);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      float2 v0, v1;
      if constexpr ((N / 8) % 16 == 0) {
        v0 = rd0[padoff(i * (N / 8))];
        v1 = rd0[REG + padoff(i * (N / 8))];
      } else {
        v0 = lds[c0 * REG + pad16(r0 + i * (N / 8))];
        v1 = lds[(c0 + 1) * REG + pad16(r0 + i * (N / 8))];
      }
      if constexpr (SP == SP_F16) dst16[i * dstep / 2] = make_uint2(pack_h2(v0.x, v0.y), pack_h2(v1.x, v1.y));
      else if constexpr (SP == SP_S48 || SGS > 0) {
        // (soffset 0: hipcc pads the store-data hazard itself here, see store_b96_padded)
        __builtin_amdgcn_raw_buffer_store_b96(s48_pack<T >= 4 ? 4 : 2>(v0, v1, c0 & (T >= 4 ? 3 : 0)), wrs,
                                              (uint32_t)((dbase + i * dstep) * sizeof(S48)), 0,
                                              kK1WriteThrough ? 16 /* sc1 */ : 0);
      }
      else if constexpr (kK1WriteThrough && N <= 4096) st_f4_wt(wrs, (uint32_t)((dbase + i * dstep) * sizeof(float2)), make_float4(v0.x, v0.y, v1.x, v1.y));
      else st_f4<kNtSpecSt>(dst + i * dstep, make_float4(v0.x, v0.y, v1.x, v1.y));
    }
  }
  if constexpr (Q15) status_add(status, n_sat);  // status word 2 (status = n_dets_dev + 2): window saturations
}

// --------------------------------------------------------------------------------------
// K1 "sequential pair" k_range_sq<N, LD, V, E> (the default at N = 4096, round 3).  T = 2 tiled
// output (the 16-B (chirp 0, chirp 1) element per range bin), the two chirps of a group going
// through ONE chirp's worth of LDS one after the other: the first chirp's spectrum waits in
// registers (V values per thread) while the second is transformed, then both are stored as 16-B
// pairs straight from registers.  Half the LDS of a two-chirp buffer doubles the workgroups per CU
// (N = 4096: three of 34 KiB), so one workgroup's barriers and LDS passes overlap another's memory
// phases.  (Round 2's "dual" kernel -- both chirps per thread in a two-chirp buffer, one workgroup
// of 8 waves per CU at N = 8192 -- was latency-bound at 0.53 of HBM and is gone since round 4.)
//   V = values per thread (16 or 32), P = N / V threads (one transform per workgroup pass);
//   E = consecutive samples per lane per load: the first pass is a radix-(V/E) Stockham pass on
//   the E groups j = E t + e, v[m] = x[j + m N/(V/E)] (E = 1: radix 16 from 8-B fp32 / 4-B fp16
//   loads, so N = 4096 = 16^3 takes two LDS exchanges instead of three; E = 2: 16-B fp32 / 8-B fp16
//   loads).  Then radix-16 LDS passes while more than V points remain per group, and the last
//   pass into registers: lane t holds X[j + m L] for j = t + P g, whole 1 KiB tiles per store
//   instruction.
// The next chirp's raw input is loaded as soon as this chirp's first pass has consumed its
// registers (one chirp ahead, whatever group it belongs to), so the load overlaps three LDS passes.
// Replaces the Xilinx range FFT (rtl/src/radar_core.vhd:303-316) + corner turner (:318-327).
// --------------------------------------------------------------------------------------
template <int N, int V> struct SqGeom {
  static constexpr int P = N / V;
  static constexpr int T = 2, RB = 64;          // = RangeGeom<N> for N >= 2048
  static constexpr int REG = padded(N);
  static constexpr int WAVES = V == 16 ? 4 : 2;  // per SIMD: 16 (V = 16) or 8 (V = 32) waves per CU
};
template <int N, typename LD, int V, int E, int W = SqGeom<N, V>::WAVES, int SP = SP_F32>
__global__ void __launch_bounds__(N / V) __attribute__((amdgpu_waves_per_eu(W)))
k_range_sq(const void* __restrict__ cube, float2* __restrict__ inter, const float* __restrict__ win,
           const float* __restrict__ chirp_w, int nc, int n_groups, float /* q15_scale */, uint32_t* /* status */) {
  using Gm = SqGeom<N, V>;
  constexpr int P = Gm::P, T = Gm::T, RB = Gm::RB;
  constexpr int M = V / E;                      // first-pass radix
  constexpr int S0 = N / M;                     // its input stride (= P E)
  constexpr int LL = vlast_L<N, M, V>();        // sub-transform size before the last pass
  constexpr int RF = N / LL, GF = V / RF;       // last pass: radix, groups per thread
  static_assert(RangeGeom<N>::T == T && RangeGeom<N>::RB == RB, "tile format of K2");
  static_assert(E == 1 || E == 2, "one or two samples per load");
  static_assert(M <= 16 && (M == 16 || E == 2), "first pass writes whole padded 16-point runs");
  __shared__ __attribute__((aligned(16))) float2 lds[Gm::REG];
  const int t0 = threadIdx.x;
  const int ncb = nc / T;

  // raw input of the next chirp to transform (E = 2: M loads of 2 samples; E = 1: M of 1)
  using RawT = std::conditional_t<E == 2, typename LD::Raw, typename LD::Raw1>;
  RawT a[M];
  float cwn = 1.f;
  // chirp q of group cb: cb T + q, or (SP_S48PS) the strided pair t + 2 p k + p q (chirp_of)
  const int lgp = __builtin_ctz(nc) - 4;
  auto fetch = [&](int g, int q) {
    const int fr = g / ncb;
    const int cb = g - fr * ncb;
    const int c = chirp_of<T, SP == SP_S48PS>(cb, q, lgp);
    const size_t chirp = (size_t)fr * nc + (size_t)c;
    const int t = opaque(t0);
#pragma unroll
    for (int m = 0; m < M; ++m) {
      if constexpr (E == 2) a[m] = LD::fetch(cube, chirp * N + 2 * t + S0 * m);
      else a[m] = LD::fetch1(cube, chirp * N + t + S0 * m);
    }
    if (chirp_w) cwn = chirp_w[__builtin_amdgcn_readfirstlane(c)];
  };
  // range window of this thread's first-pass samples, held (V floats)
  float wh[V];
#pragma unroll
  for (int m = 0; m < M; ++m) {
    if constexpr (E == 2) {
      const float2 w2 = *reinterpret_cast<const float2*>(win + 2 * t0 + S0 * m);
      wh[2 * m] = w2.x;
      wh[2 * m + 1] = w2.y;
    } else {
      wh[m] = win[t0 + S0 * m];
    }
  }
#pragma unroll
  for (int i = 0; i < V; ++i) asm volatile("" ::"v"(wh[i]));  // complete before the loop (vmcnt order)

  int g = blockIdx.x;
  if (g < n_groups) fetch(g, 0);
  for (; g < n_groups; g += gridDim.x) {
    const int fr = g / ncb;
    const int cb = g - fr * ncb;
    float2 X[2][GF][RF];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int t = opaque(t0);
      const float cw = cwn;
      __syncthreads();  // the previous transform's last-pass reads are done with lds
      // first pass from registers: window (x Doppler weight of the chirp), radix M, E groups
#pragma unroll
      for (int e = 0; e < E; ++e) {
        float2 v[M];
#pragma unroll
        for (int m = 0; m < M; ++m) {
          float2 x;
          if constexpr (E == 2) {
            const float4 x4 = LD::expand(a[m]);
            x = e ? make_float2(x4.z, x4.w) : make_float2(x4.x, x4.y);
          } else {
            x = LD::expand1(a[m]);
          }
          const float we = wh[E * m + e] * cw;
          v[m] = make_float2(x.x * we, x.y * we);
        }
        Dft<M>::run(v);
        float2* d = lds + pad16((E * t + e) * M);
#pragma unroll
        for (int m = 0; m < M; ++m) d[m] = v[m];
      }
      // the next chirp's input: this group's second chirp, or the next group's first
      if (q == 0) fetch(g, 1);
      else if (g + (int)gridDim.x < n_groups) fetch(g + gridDim.x, 0);
      __syncthreads();
      vpasses_mid<N, M, P, V>(lds, t);
      vpass_last<N, LL, P, V>(lds, t, X[q]);
    }
    // tile stores: lane t holds range bins d = t + P gg + LL m of both chirps; write-through (sc1)
    // at N <= 4096 as k_range: no dirty spectrum lines left in L2 for the end-of-kernel release
    // (config 3: K1 58.3-58.7 -> 57.2-57.6 us per launch, 21.7-21.8 k -> 22.0-22.1 k frames/s,
    // profiles/r04/k1/policy/; nt + sc1 7 % slower)
    // (SP_S48: the pair form, 12 B per element, same policy)
    const int t = opaque(t0);
    const size_t fbase = (size_t)fr * N * nc;
    constexpr bool WT = kK1WriteThrough && N <= 4096;
    constexpr bool S48V = SP == SP_S48 || SP == SP_S48PS;  // (S48 names the point struct)
    constexpr size_t EB = S48V ? sizeof(S48) : sizeof(float2);  // bytes per point
    const __amdgpu_buffer_rsrc_t srs =  // one frame's tiles < 4 GiB
        S48V ? wt_rsrc(reinterpret_cast<char*>(inter) + fbase * EB, 0xffffffffu) : wt_rsrc(inter + fbase, 0xffffffffu);
#pragma unroll
    for (int gg = 0; gg < GF; ++gg)
#pragma unroll
      for (int m = 0; m < RF; ++m) {
        const int d = t + P * gg + LL * m;
        const size_t off = ((size_t)(d / RB) * ncb + cb) * (RB * T) + (size_t)(d % RB) * T;
        if constexpr (S48V) {
          __builtin_amdgcn_raw_buffer_store_b96(s48_pack<2>(X[0][gg][m], X[1][gg][m], 0), srs, (uint32_t)(off * EB), 0,
                                                WT ? 16 /* sc1 */ : 0);  // (soffset 0: padded by hipcc)
        } else {
          const float4 x = make_float4(X[0][gg][m].x, X[0][gg][m].y, X[1][gg][m].x, X[1][gg][m].y);
          if constexpr (WT) st_f4_wt(srs, (uint32_t)(off * sizeof(float2)), x);
          else st_f4<kNtSpecSt>(inter + fbase + off, x);
        }
      }
  }
}

// --------------------------------------------------------------------------------------
// K1 "permlane pair" k_range_px<LD> for N = 8192 (round 3): k_range_sq's sequential pair with
// 16 values per thread (512 threads, one 68 KiB transform buffer, two workgroups per CU), but
// 8192 = 16 x 16 x 16 x 2 with two LDS exchanges instead of three:
//   pass A  radix 16 from registers (one fp16/int16/fp32 sample per lane per load, stride 512),
//           window x Doppler weight fused, written to LDS;
//   pass B  radix 16 through LDS (sub-transforms 16 -> 256);
//   pass C  radix 16 read from LDS into registers (256 -> 4096), thread (lane l, wave w) taking
//           j = (l & 31) + 32 w + 256 (l >> 5): the two half-waves hold the two 4096-point
//           halves y0, y1 at the same offsets k + 256 m;
//   pass D  the last radix-2 (4096 -> 8192) between the half-waves: v_permlane32_swap of
//           registers m and m + 8 leaves each lane 8 complete (y0, y1) pairs, p = k + 256 m',
//           m' = m + 8 (1 - h), X[p] = y0 + W^p y1, X[p + 4096] = y0 - W^p y1.
// (Measured and dropped: pass B inside each wave -- lane (w, l) playing pass-A thread u + 32 i and
// pass-B thread 16 u + i, u = 4 w + (l >> 4), i = l & 15, so the A -> B exchange needs no barrier
// -- makes every pass-A load instruction read 16-B runs of 16 lines: 132 us per 3-frame launch
// (105 us with cached loads) against 58 us, profiles/r03/k1px/k1lab_c5_3f_wl.log.)
// The first chirp's 16 outputs wait in registers while the second is transformed, then both go out
// as 16-B (chirp 0, chirp 1) tile elements: lanes 0-31 and 32-63 each write 512 contiguous bytes.
// Replaces the Xilinx range FFT (rtl/src/radar_core.vhd:303-316) + corner turner (:318-327).
// --------------------------------------------------------------------------------------
__device__ __forceinline__ void swap32(float2& a, float2& b) {
  // a, b := [a_lo, b_lo], [a_hi, b_hi] (lo / hi = lanes 0-31 / 32-63)
  const auto rx = __builtin_amdgcn_permlane32_swap(__float_as_uint(a.x), __float_as_uint(b.x), false, false);
  const auto ry = __builtin_amdgcn_permlane32_swap(__float_as_uint(a.y), __float_as_uint(b.y), false, false);
  a = make_float2(__uint_as_float(rx[0]), __uint_as_float(ry[0]));
  b = make_float2(__uint_as_float(rx[1]), __uint_as_float(ry[1]));
}
// (Measured and dropped: an XOR-swizzled unpadded layout in which pass A stores into exactly the
// slots its own lane read in the previous pass C, so the barrier between them goes (3 per chirp):
// 64.9 vs 59.3 us per 3-frame launch, equal at 12 frames -- profiles/r03/k1px/k1lab_c5_sw.log.)
// WS: range-window values per thread kept in LDS instead of VGPRs (the last WS of the 16).  At 128
// VGPRs (4 waves per SIMD) the kernel otherwise spills a window value to scratch, and its reload --
// a vector-memory op issued after the group's 16 tile stores -- makes the next group's pass A wait,
// in vmcnt order, for every one of those stores.  68 + 2 WS KiB of LDS per workgroup: two still fit
// a CU (160 KiB) up to WS = 6.
template <typename LD, int W = 4, int WS = 4, int SP = SP_F32>
__global__ void __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(W)))
k_range_px(const void* __restrict__ cube, float2* __restrict__ inter, const float* __restrict__ win,
           const float* __restrict__ chirp_w, int nc, int n_groups, float /* q15_scale */, uint32_t* /* status */) {
  constexpr int N = 8192, T = 2, RB = 64;
  static_assert(RangeGeom<N>::T == T && RangeGeom<N>::RB == RB, "tile format of K2");
  static_assert(WS >= 0 && WS <= 6, "two workgroups per CU");
  __shared__ __attribute__((aligned(16))) float2 lds[padded(N)];
  __shared__ float wlds[WS > 0 ? WS * 512 : 1];
  const int t0 = threadIdx.x;
  const int lane = t0 & 63, wv = t0 >> 6, h = lane >> 5;
  const int ncb = nc / T;

  // loads and stores through buffer descriptors: one lane offset, the m-dependent part in the
  // SGPR offset (no 64-bit address per load / store in VGPRs)
  using Raw1 = typename LD::Raw1;
  constexpr int SB = sizeof(Raw1);  // bytes per sample
  constexpr int NTL = kNtCube ? 2 : 0;  // non-temporal cube loads (read once)
  Raw1 a[16];
  float cwn = 1.f;
  // chirp q of group cb: cb T + q, or (SP_S48PS) the strided pair t + 2 p k + p q (chirp_of)
  const int lgp = __builtin_ctz(nc) - 4;
  auto fetch = [&](int g, int q) {
    const int fr = g / ncb;
    const int cb = g - fr * ncb;
    const int c = chirp_of<T, SP == SP_S48PS>(cb, q, lgp);
    const size_t chirp = (size_t)fr * nc + (size_t)c;
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<char*>(reinterpret_cast<const char*>(cube)) + chirp * N * SB, (short)0, N * SB, 0x00020000);
    const int vo = opaque(t0) * SB;
#pragma unroll
    for (int m = 0; m < 16; ++m) {
      if constexpr (SB == 4) {
        a[m] = __builtin_bit_cast(Raw1, __builtin_amdgcn_raw_buffer_load_b32(rs, vo, m * 512 * SB, NTL));
      } else {
        a[m] = __builtin_bit_cast(Raw1, __builtin_amdgcn_raw_buffer_load_b64(rs, vo, m * 512 * SB, NTL));
      }
    }
    if (chirp_w) cwn = chirp_w[__builtin_amdgcn_readfirstlane(c)];
  };
  float wh[16 - WS];  // range window of samples t + 512 m, held (m < 16 - WS; the rest in wlds)
#pragma unroll
  for (int m = 0; m < 16 - WS; ++m) wh[m] = win[t0 + 512 * m];
#pragma unroll
  for (int m = 16 - WS; m < 16; ++m) wlds[(m - 16 + WS) * 512 + t0] = win[t0 + 512 * m];
#pragma unroll
  for (int i = 0; i < 16 - WS; ++i) asm volatile("" ::"v"(wh[i]));  // complete before the loop (vmcnt order)

  // pass C's group j = kc + 256 h; the pass-D twiddle base W_8192^(kc + 2048 (1 - h))
  const int kc = (lane & 31) + 32 * wv;
  const float2 cd = twiddle<N>(kc + 2048 * (1 - h));

  int g = blockIdx.x;
  if (g < n_groups) fetch(g, 0);
  for (; g < n_groups; g += gridDim.x) {
    const int fr = g / ncb;
    const int cb = g - fr * ncb;
    float2 X[2][16];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int t = opaque(t0);
      const float cw = cwn;
      __syncthreads();  // the previous transform's pass-C reads are done with lds
      {  // pass A: window, radix 16 over x[t + 512 m]
        float2 v[16];
#pragma unroll
        for (int m = 0; m < 16; ++m) {
          const float w = m < 16 - WS ? wh[m < 16 - WS ? m : 0] : wlds[(m - 16 + WS) * 512 + t];
          v[m] = LD::expand1_scaled(a[m], w * cw);
        }
        Dft<16>::run(v);
        float2* d = lds + pad16(16 * t);
#pragma unroll
        for (int m = 0; m < 16; ++m) d[m] = v[m];
      }
      // the next chirp's input: this group's second chirp, or the next group's first
      if (q == 0) fetch(g, 1);
      else if (g + (int)gridDim.x < n_groups) fetch(g + gridDim.x, 0);
      {  // pass B: radix 16, L = 16 (in place, barriers around the exchange)
        __syncthreads();
        float2 v[16];
        const float2* src = lds + pad16(t);
#pragma unroll
        for (int m = 0; m < 16; ++m) v[m] = src[padoff(m * 512)];
        __syncthreads();
        const int k = t & 15;
        GroupTwiddles<16, 256> tb;
        tb.init(k);
#pragma unroll
        for (int m = 1; m < 16; ++m) v[m] = cmul(v[m], tb.pow(m));
        Dft<16>::run(v);
        float2* dst = lds + pad16((t >> 4) * 256 + k);
#pragma unroll
        for (int m = 0; m < 16; ++m) dst[padoff(m * 16)] = v[m];
        __syncthreads();
      }
      {  // pass C: radix 16, L = 256, into registers; v[m] = y_h[kc + 256 m]
        float2* v = X[q];
        const float2* src = lds + pad16(opaque(kc + 256 * h));
#pragma unroll
        for (int m = 0; m < 16; ++m) v[m] = src[padoff(m * 512)];
        GroupTwiddles<16, 4096> tc;
        tc.init(opaque(kc));
#pragma unroll
        for (int m = 1; m < 16; ++m) v[m] = cmul(v[m], tc.pow(m));
        float2 cdl = cd;  // per chirp: the W_32^m products below must not be hoisted (14 VGPRs)
        asm volatile("" : "+v"(cdl.x), "+v"(cdl.y));
        Dft<16>::run(v);
        // pass D: radix 2 between the half-waves; X[q][m + 8] = y0[p], X[q][m] = y1[p] ->
        // X[q][m + 8] = X[p], X[q][m] = X[p + 4096], p = kc + 256 (m + 8 (1 - h))
#pragma unroll
        for (int m = 0; m < 8; ++m) {
          swap32(v[m + 8], v[m]);
          // W_8192^(p) = cd * W_32^m
          const float2 w32 = make_float2(__builtin_cosf(2.0f * 3.14159265358979323846f * m / 32.f),
                                         -__builtin_sinf(2.0f * 3.14159265358979323846f * m / 32.f));
          const float2 tw = m ? cmul(cdl, w32) : cdl;
          const float2 b = cmul(v[m], tw);
          const float2 a0 = v[m + 8];
          v[m + 8] = cadd(a0, b);
          v[m] = csub(a0, b);
        }
      }
    }
    // tile stores: lane holds X[d] of both chirps for d = p (register m + 8) and p + 4096 (m)
    // d / 64 = (w >> 1) + 4 m' + 64 s, d % 64 = (l & 31) + 32 (w & 1); tile (d / 64, cb) is 1 KiB
    // (SP_S48: the pair form, 12-B elements in 768-B tiles)
    constexpr bool S48V = SP == SP_S48 || SP == SP_S48PS;  // (S48 names the point struct)
    constexpr int EB = S48V ? 2 * (int)sizeof(S48) : 16;  // bytes per (chirp 0, chirp 1) element
    void* const fbase = S48V ? static_cast<void*>(reinterpret_cast<char*>(inter) + (size_t)fr * N * nc * (EB / 2))
                                     : static_cast<void*>(inter + (size_t)fr * N * nc);
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(fbase, (short)0, N * nc * (EB / 2), 0x00020000);
    const int t = opaque(t0);
    const int l = t & 63, w = t >> 6;
    const int vo = (((w >> 1) + 32 * (1 - (l >> 5))) * ncb + cb) * (64 * EB) + ((l & 31) + 32 * (w & 1)) * EB;
#pragma unroll
    for (int m = 0; m < 8; ++m)
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const int r = s ? m : m + 8;
        if constexpr (S48V) {
          store_b96_padded<0 /* write-back */>(s48_pack<2>(X[0][r], X[1][r], 0), rs, (uint32_t)vo,
                                               (4 * m + 64 * s) * ncb * (64 * EB));
        } else {
          typedef float f4v __attribute__((ext_vector_type(4)));
          const f4v x = {X[0][r].x, X[0][r].y, X[1][r].x, X[1][r].y};
          __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(fmcw_u4v, x), rs, vo,
                                                 (4 * m + 64 * s) * ncb * (64 * EB), 0 /* write-back */);
        }
      }
  }
}

}  // namespace fmcw
