// doppler_kernel.hpp -- K2 k_doppler: Doppler window + FFT + |X| / NCI + map + 1-D OS-CFAR.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cfar1d.hpp"
#include "det_sink.hpp"
#include "fft_device.hpp"
#include "spectrum.hpp"

namespace fmcw {

// --------------------------------------------------------------------------------------
// K2: Doppler window + FFT + magnitude (+NCI over rx) + map + 1-D OS-CFAR, one wave tile at a
// time (see "Wave tiles", cfar1d.hpp).  Lane (rr, t) of P = NC/16 owns range row r0 + rr's
// transform.  Pass 1 (radix 16, no twiddles) reads its 16 points c = t + P m straight from
// the tiled spectrum (8-byte loads: two 256-B runs per load instruction across the wave's
// rows and lanes); the Doppler window was already applied by K1 (MTI off) or is applied here
// after the canceller (MTI on); the last pass stays in registers and feeds |X|^2 (summed over
// rx: NCI) directly.
// --------------------------------------------------------------------------------------
// FMCW_COMPAT_MTI word format: round half to even (the IP's convergent rounding) and saturate
// to int16, per component; and the canceller's output saturation (doppler_notch.vhd:75-93).
__device__ __forceinline__ float sat16(float v) { return fminf(fmaxf(v, -32768.f), 32767.f); }
__device__ __forceinline__ float2 sat16c(float2 v) { return make_float2(sat16(v.x), sat16(v.y)); }
__device__ __forceinline__ float2 q16c(float2 v) { return make_float2(sat16(rintf(v.x)), sat16(rintf(v.y))); }
// the same, counting a sample whose I or Q clipped
__device__ __forceinline__ float2 q16c_count(float2 v, uint32_t& n) {
  const float2 r = make_float2(rintf(v.x), rintf(v.y)), q = sat16c(r);
  n += (uint32_t)(q.x != r.x || q.y != r.y);
  return q;
}
__device__ __forceinline__ float2 sat16c_count(float2 v, uint32_t& n) {
  const float2 q = sat16c(v);
  n += (uint32_t)(q.x != v.x || q.y != v.y);
  return q;
}
// RTL-compat Q15 window on an int16 word pair: y = sat16(floor((x c + 2^14) / 2^14)) per
// component (window_multiplier.vhd:126-158), c = the ROM integer; x c < 2^31 for int16 words.
__device__ __forceinline__ float2 win_q15c(float2 x, float c, uint32_t& n) {
  const int ci = (int)c;
  const int yi = ((int)x.x * ci + (1 << 14)) >> 14, yq = ((int)x.y * ci + (1 << 14)) >> 14;
  const int si = min(max(yi, -32768), 32767), sq = min(max(yq, -32768), 32767);
  n += (uint32_t)(si != yi || sq != yq);
  return make_float2((float)si, (float)sq);
}

// Workgroups are dispatched round-robin over the 8 XCDs (XCD = id % 8, MI355X_MICROARCH.md).
// Giving each XCD a contiguous range of logical ids puts neighbouring tiles -- which read the
// two halves of the same 128-B lines of the tiled spectrum when a workgroup covers only 64 B of
// each 1 KiB tile (NC = 1024: 4 range rows x 16 B) -- behind the same L2.
__device__ __forceinline__ int xcd_block_id(int bid, int grid) {
  if (grid & 7) return bid;
  return (bid & 7) * (grid >> 3) + (bid >> 3);
}

// K2's register prefetch of the next (tile, rx) unit (MTI off), points loaded ahead: all 16 up to
// NC = 256; 8 (half a unit) at NC = 512, which fits 165 instead of 178 VGPRs and so 3 waves per
// SIMD (config-3 K2 41.6-41.9 -> 39.0-39.2 us per launch, profiles/r03/k2/k2_pf_ab.log; 16 points
// 42.1, none 42.2-42.5); none at NC = 1024 (8 or 16 points: 61-64 against 56 us).
template <int NC, int MTI>
// (Round 6, config 3: 4 points ahead 38.4-38.9 against 35.8-35.9 us per launch, profiles/r06/k2_c3_ab/.)
constexpr int k2_prefetch() { return MTI != 0 ? 0 : NC <= 256 ? 16 : NC == 512 ? 8 : 0; }
// FAST (below) at NC = 256 fits 128 VGPRs without scratch: 4 waves per SIMD (4 workgroups of
// 39 KiB LDS per CU); measured K2 58.2 -> 56.0 us per 96-frame launch at config 2.  At NC = 512
// / 1024 the fourth wave costs more than it hides (config 3 K2 41.7 -> 55.9 us, config 5 55.5
// -> 74.6 us per launch; gpurun_out bench_libs, round 2).  The S48 FAST K2 at NC = 256: 4 waves
// (128 VGPRs, 16 B of scratch) measured 0.570 us per frame, 3 waves 0.584-0.598, an 8-point
// prefetch 0.571-0.574 (profiles/r05/spec_ab/).
template <int NC, int MTI, bool FAST = false>
constexpr int k2_waves() { return (FAST && MTI == 0 && NC == 256) ? 4 : 2; }
// FAST: the common configuration fixed at compile time -- |X| magnitude (no AMBM), no dB map,
// and the 1-D CFAR, when enabled, at the reference geometry (8 refs / 2 guards per side, need =
// n_ref - rank <= 4, fp32 compare).  The generic kernel keeps those as uniform runtime branches,
// whose other arms held registers and SGPRs (spills to VGPR lanes) across the tile loop.
// SP: the spectrum format K1 wrote (SP_F32, SP_F16, SP_S48 quad form (T >= 8, P % 4 == 0), SP_S48S / SP_S48PS
// pair form (T = 2, P % 2 == 0); S48 with MTI off).
template <int NC, int MTI, int SP = SP_F32, bool FAST = false>
__global__ void __launch_bounds__(DopplerGeom<NC>::NT) __attribute__((amdgpu_waves_per_eu(k2_waves<NC, MTI, FAST>())))
k_doppler(const float2* __restrict__ inter_in, const float* __restrict__ win_d, int ns, int nrx,
          int lgT, int lgRB, int n_tiles, int frame0, int tile0, float* __restrict__ lin_map,
          float* __restrict__ db_map, int mag_mode, int mti_rtl, int q15d, Cfar1DArgs cf, DetSink sink,
          uint32_t* __restrict__ status) {
  using Gm = DopplerGeom<NC>;
  constexpr int P = Gm::P, WR = Gm::WR, WPB = Gm::WPB, REGD = Gm::REGD, REGM = Gm::REGM;
  constexpr int LR = Gm::LR, LG = Gm::LG;
  static_assert(P <= 64, "a Doppler transform must fit one wave");
  __shared__ __attribute__((aligned(16))) float lds[WPB * Gm::WFL];

  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane0 = threadIdx.x & 63;
  using SE = typename SpecEl<SP>::T;
  const SE* const inter = reinterpret_cast<const SE*>(inter_in);
  const float sscale = SP == SP_F16 ? (float)ns : 1.f;  // undoes K1's 1 / N_range of an fp16 spectrum
  constexpr int SGS = s48_strided_g<SP>();  // strided S48: a lane's SGS points per element (no exchange)
  constexpr bool S48S = SGS > 0;
  constexpr bool S48F = SP == SP_S48;  // adjacent quads: exponent pieces ORed over a lane quad
  constexpr int SG = 4;
  static_assert(!S48F || (MTI == 0 && P % SG == 0), "S48: a lane group holds a chirp group");
  static_assert(!S48S || MTI == 0, "S48: MTI off");
  // S48: this lane's chirps c = t + P m all sit at c % G = t % G of their group (t = lane % P);
  // the two lane constants are derived from t where they are used (not held across the loop)
  auto s48_sh = [](int tt) { return (uint32_t)(tt & 1) << 4; };   // byte offset x 8 of the record in its load
  auto s48_qs = [](int tt) { return (uint32_t)(tt & (SG - 1)) * (8 / SG); };  // its exponent piece's shift
  const int rr = lane0 / P;
  const int t0 = lane0 % P;
  float* const mags = lds + wv * Gm::WFL;
  float2* const wreg = reinterpret_cast<float2*>(mags);
  uint32_t* const list = reinterpret_cast<uint32_t*>(mags + Gm::LIST);
  const int tiles_per_frame = ns / WR;
  const int nf = n_tiles / tiles_per_frame;
  const int T = 1 << lgT;
  const int lgncb = __builtin_ctz(NC) - lgT;
  // Doppler window for this lane's chirps c = t + P m.  MTI off: K1 already applied it
  // (chirp_w), so no registers are spent on it here.  MTI on: the canceller must see the
  // unwindowed spectrum (doppler_notch precedes doppler_fft, radar_core.vhd:329-352).
  // q15d (FMCW_WIN_Q15_RTL, generic kernel only): win_d holds the ROM integers c[n] and the
  // window is the RTL's integer arithmetic on the spectrum's int16 words, applied here.
  constexpr bool WIN_K2 = MTI != 0 || !FAST;
  float wv_d[WIN_K2 ? 16 : 1];
  if constexpr (WIN_K2) {
    if (MTI != 0 || q15d) {
#pragma unroll
      for (int m = 0; m < 16; ++m) wv_d[m] = win_d[t0 + P * m];
    }
  }
  uint32_t n_wsat = 0, n_msat = 0;  // saturated samples: integer Doppler window; int16 words / MTI

  // element (r, c) of the tiled spectrum: ((rb*NCB + c/T)*RB + r%RB)*T + c%T
  auto off_of = [&](uint32_t rbase, uint32_t rin, uint32_t c) -> uint32_t {
    return ((((rbase + (c >> lgT)) << lgRB) + rin) << lgT) | (c & (uint32_t)(T - 1));
  };

  // Software pipeline (MTI off): the 16 points of the next (tile, rx) unit are loaded into
  // registers right after this unit's first pass has consumed its own, so a wave keeps 8 KiB
  // of HBM reads in flight through its FFT, magnitude, map store and CFAR phases instead of
  // exposing the full load latency once per unit.
  constexpr int NPF = k2_prefetch<NC, MTI>();  // points loaded ahead
  constexpr bool PF = NPF > 0;
  // Tile order: the WPB waves of a workgroup take WPB consecutive wave tiles (row groups) of one
  // frame, frame-minor over workgroups, so the 4 x WR rows they read from each 1 KiB block of the
  // tiled spectrum are requested together (DRAM page locality; round 1, config 2: K2 0.905 ->
  // 0.874 us/frame against frame-minor over all waves, which remains for frames whose tile count
  // is not a multiple of WPB).
  const bool grp = tiles_per_frame % WPB == 0;
  auto tile_fl = [&](int tl, int& fo, int& lo) {
    if (grp) {
      const int u = tl / WPB;
      fo = u % nf;
      lo = (u / nf) * WPB + (tl % WPB);
    } else {
      fo = tl % nf;
      lo = tl / nf;
    }
  };
  const int tile_step = gridDim.x * WPB;
  auto unit_src = [&](int tl, int rx) -> const SE* {
    int fu, lu;
    tile_fl(tl, fu, lu);
    const int ru = lu * WR + rr;
    return inter + ((size_t)fu * nrx + rx) * (size_t)ns * NC +
           off_of((uint32_t)(ru >> lgRB) << lgncb, (uint32_t)(ru & ((1 << lgRB) - 1)), 0);
  };
  float2 nxt[PF && !S48S ? NPF : 1];  // prefetched points (S48 quads: the raw 8 bytes)
  fmcw_u3v nxq[PF && S48S ? NPF / 2 : 1];  // strided S48: 12-B loads (a quad's halves, or a pair)
  const __amdgpu_buffer_rsrc_t srs = wt_rsrc(const_cast<SE*>(inter), 0xffffffffu);  // the prefetch's buffer loads
  // last-pass twiddle bases, once per lane (NC = 256: pass 1 + one radix-16 pass, k = t)
  constexpr bool TWH = NC / 16 <= 16 && P % 16 == 0;
  GroupTwiddles<NC / 16, NC> twh;
  if constexpr (TWH) twh.init(t0 & 15);
  auto prefetch = [&](int tl, int rx) {
    if constexpr (PF) {
      if (tl < n_tiles) {
        const SE* p = unit_src(tl, rx);
        const int tq = opaque(t0);
        if constexpr (S48S) {
          // group k of lane t: K1 group cb = t + P k of the row block, element j = 0; groups P apart
          const uint32_t vo = (uint32_t)((const char*)(p + (((uint32_t)tq << lgRB) << lgT)) - (const char*)inter);
          const uint32_t sb = (((uint32_t)P << lgRB) << lgT) * (uint32_t)sizeof(S48);
          uint32_t so = 0;
#pragma unroll
          for (int k = 0; k < NPF / SGS; ++k) {
#pragma unroll
            for (int h = 0; h < SGS / 2; ++h)
              nxq[(SGS / 2) * k + h] = __builtin_bit_cast(fmcw_u3v, __builtin_amdgcn_raw_buffer_load_b96(srs, vo, so + 12u * h, 0));
            so += sb;
            asm volatile("" : "+s"(so));
          }
        } else if ((P & (T - 1)) == 0) {  // uniform: chirps t + P m sit a fixed S elements apart
          const SE* pb = p + ((((uint32_t)tq >> lgT) << lgRB) << lgT) + ((uint32_t)tq & (uint32_t)(T - 1));
          const uint32_t S = (uint32_t)(P >> lgT) << (lgRB + lgT);
          // the uniform m S byte offsets, one SGPR advanced per load: left to the compiler, the 16
          // products were hoisted out of the tile loop and held in 16 SGPRs, which pushed 25
          // others into VGPR lanes (a v_readlane per use inside the loop)
          uint32_t so = 0;
          const uint32_t sb = S * (uint32_t)sizeof(SE);
#pragma unroll
          for (int m = 0; m < NPF; ++m) {
            if constexpr (S48F) {
              // the raw 8 bytes at the point's record rounded down to 4 (decoded at use)
              const uint32_t vo = (uint32_t)((const char*)pb - (const char*)inter) - (s48_sh(tq) >> 3);
              typedef float f2v __attribute__((ext_vector_type(2)));
              const f2v r = __builtin_bit_cast(
                  f2v, __builtin_amdgcn_raw_buffer_load_b64(srs, vo, so, kNtSpecLd ? 2 /* nt */ : 0));
              nxt[m] = make_float2(r.x, r.y);
              so += sb;
              asm volatile("" : "+s"(so));
            } else if constexpr (SP == SP_F32) {
              // buffer load: lane offset in a VGPR, the uniform m S in an SGPR (no 64-bit VALU
              // address add per load; the chunk's spectrum is < 4 GiB, fmcw_create caps it)
              const uint32_t vo = (uint32_t)((const char*)pb - (const char*)inter);
              typedef float f2v __attribute__((ext_vector_type(2)));
              const f2v r = __builtin_bit_cast(
                  f2v, __builtin_amdgcn_raw_buffer_load_b64(srs, vo, so, kNtSpecLd ? 2 /* nt */ : 0));
              nxt[m] = make_float2(r.x, r.y);
              so += sb;
              asm volatile("" : "+s"(so));
            } else {
              nxt[m] = ld_spec<kNtSpecLd>(pb + (size_t)m * S, sscale);
            }
          }
        } else {
#pragma unroll
          for (int m = 0; m < NPF; ++m) {
            const uint32_t c = (uint32_t)(tq + P * m);
            const SE* pc = p + ((((c >> lgT) << lgRB) << lgT) | (c & (uint32_t)(T - 1)));
            if constexpr (S48F) {
              const fmcw_u2v r = ld_s48_raw<kNtSpecLd>(pc, (uint32_t)tq & 1u);
              nxt[m] = make_float2(__uint_as_float(r.x), __uint_as_float(r.y));
            } else {
              nxt[m] = ld_spec<kNtSpecLd>(pc, sscale);
            }
          }
        }
      }
    }
  };
  // XCD-contiguous ids only where a workgroup reads less than a 128-B line of each tile
  // (measured: config 5 K2 177 -> 110 us per 4 frames; configs 2 / 3, whose workgroups read
  // whole lines, 2-3 % slower with it)
  // (S48: its 6-B points, so config 3's 96-B reads take the XCD mapping too)
  // (round 6, config 3 with the remap: K2 37.0-37.9 against 35.8-35.9 us per launch, profiles/r06/k2_c3_ab/)
  const bool xcd = ((WPB * WR * (S48F || S48S ? 6 : 8)) << lgT) < 128;
  const int bid = xcd ? xcd_block_id((int)blockIdx.x, (int)gridDim.x) : (int)blockIdx.x;
  prefetch(bid * WPB + wv, 0);

  for (int tile = bid * WPB + wv; tile < n_tiles; tile += tile_step) {
    const int t = opaque(t0);
    float2* buf = wreg + rr * REGD;
    // frame-minor order: consecutive tiles are the same rows of consecutive frames, so the
    // rows that hold a target (more candidates, more detections) spread over all waves
    int f, lt;                                   // frame, wave tile within the frame
    tile_fl(tile, f, lt);
    const int r0 = lt * WR;
    const int r = r0 + rr;
    const uint32_t rbase = (uint32_t)(r >> lgRB) << lgncb;
    const uint32_t rin = (uint32_t)(r & ((1 << lgRB) - 1));
    float acc[LG][LR];
#pragma unroll
    for (int g = 0; g < LG; ++g)
#pragma unroll
      for (int m = 0; m < LR; ++m) acc[g][m] = 0.f;

    for (int rx = 0; rx < nrx; ++rx) {
      const SE* src = inter + ((size_t)f * nrx + rx) * (size_t)ns * NC;
      auto at = [&](uint32_t c) -> float2 {
        if constexpr (S48S) return make_float2(0.f, 0.f);  // (unused: the points come from vq)
        else if constexpr (S48F) return s48_unpack<SG>(ld_s48_raw<kNtSpecLd>(src + off_of(rbase, rin, c), c & 1u), (uint32_t)t & 1u, s48_qs(t));
        else return ld_spec<kNtSpecLd>(src + off_of(rbase, rin, c), sscale);
      };
      float2 v[16];
      // strided S48: all 16 points decoded here, SGS per element, prefetched or loaded now
      float2 vq[S48S ? 16 : 1];
      if constexpr (S48S) {
        const uint32_t q_vo = (uint32_t)((const char*)(src + off_of(rbase, rin, (uint32_t)t << lgT)) - (const char*)inter);
        const uint32_t q_sb = (((uint32_t)P << lgRB) << lgT) * (uint32_t)sizeof(S48);
#pragma unroll
        for (int k = 0; k < 16 / SGS; ++k) {
          fmcw_u3v w[SGS / 2];
#pragma unroll
          for (int h = 0; h < SGS / 2; ++h) {
            if (SGS * k < NPF) w[h] = nxq[SGS * k < NPF ? (SGS / 2) * k + h : 0];
            else w[h] = __builtin_bit_cast(fmcw_u3v, __builtin_amdgcn_raw_buffer_load_b96(srs, q_vo, (uint32_t)k * q_sb + 12u * h, 0));
          }
          if constexpr (SGS == 4) {
            float2 o[4];
            s48s_unpack4(w[0], w[SGS / 2 - 1], o);
#pragma unroll
            for (int j = 0; j < 4; ++j) vq[4 * k + j] = o[j];
          } else {
            float2 o[2];
            s48ps_unpack2(w[0], o);
            vq[2 * k] = o[0];
            vq[2 * k + 1] = o[1];
          }
        }
      }
#pragma unroll
      for (int m = 0; m < 16; ++m) {
        const int c = t + P * m;
        float2 x;
        if (S48S) {
          x = vq[S48S ? m : 0];
        } else if (m < NPF) {
          x = nxt[m < NPF && !S48S ? m : 0];
          if constexpr (S48F) x = s48_unpack<SG>(fmcw_u2v{__float_as_uint(x.x), __float_as_uint(x.y)}, (uint32_t)t & 1u, s48_qs(t));
        } else {
          x = at((uint32_t)c);
        }
        // RTL-compat words: the corner turner hands the FFT IP's 16-bit output words on
        // (round half to even, saturate; counted in status word 3)
        const bool words = !FAST && (mti_rtl || q15d);
        if (words) x = q16c_count(x, n_msat);
        if constexpr (MTI >= 2) {  // MTI canceller along slow time, zero history (doppler_notch.vhd:72-102)
          float2 x1 = c >= 1 ? at((uint32_t)(c - 1)) : make_float2(0.f, 0.f);
          float2 x2 = make_float2(0.f, 0.f);
          if constexpr (MTI == 3) x2 = c >= 2 ? at((uint32_t)(c - 2)) : make_float2(0.f, 0.f);
          if (words) {  // 16-bit words in (their own clipping was counted at their own chirp)
            x1 = q16c(x1);
            x2 = q16c(x2);
          }
          // integers below 2^18 on words: every step below is exact
          x = MTI == 2 ? csub(x, x1) : cadd(csub(x, cscale(x1, 2.f)), x2);
          if (words) x = sat16c_count(x, n_msat);  // the canceller's saturating output (:76-93)
        }
        if constexpr (WIN_K2) {
          if (!FAST && q15d) x = win_q15c(x, wv_d[m], n_wsat);  // window_multiplier.vhd:146-158
          else if (MTI != 0) x = cscale(x, wv_d[m]);
        }
        v[m] = x;
      }
      Dft<16>::run(v);                       // pass 1: L = 1, no twiddles
      {
        float2* d = buf + pad16(16 * t);     // y[16 t + m]
#pragma unroll
        for (int m = 0; m < 16; ++m) d[m] = v[m];
      }
      pass_sync<false>();
      {
        // one prefetch site: two (one per branch) merged their register results through copies
        // (round 6: issued right after the strided-S48 decode instead, config 2 K2 measured 64.5-67.8
        // against 64.7-65.3 us per launch, profiles/r06/k2_early_pf/)
        const bool same = rx + 1 < nrx;
        prefetch(same ? tile : tile + tile_step, same ? rx + 1 : 0);
      }
      float2 X[LG][LR];
      if constexpr (TWH) stockham_last_tw<NC, 16, P>(buf, t, X, twh);
      else stockham_to_regs<NC, 16, P, false>(buf, t, X);
      if (!FAST && mag_mode == FMCW_MAG_AMBM) {  // uniform: one branch for the whole block
#pragma unroll
        for (int g = 0; g < LG; ++g)
#pragma unroll
          for (int m = 0; m < LR; ++m) {
            const float ai = fabsf(X[g][m].x), aq = fabsf(X[g][m].y);
            const float mx = fmaxf(ai, aq), mn = fminf(ai, aq);
            acc[g][m] = mx + floorf(mn * 0.25f) + floorf(mn * 0.125f);
          }
      } else {
#pragma unroll
        for (int g = 0; g < LG; ++g)
#pragma unroll
          for (int m = 0; m < LR; ++m) acc[g][m] = rx == 0 ? cabs2(X[g][m]) : acc[g][m] + cabs2(X[g][m]);
      }
      pass_sync<false>();  // every read of the last pass is issued: the rows may be rewritten
    }
    // magnitudes -> the wave region (over the dead FFT rows), for the map store and the CFAR
    const bool ambm = !FAST && mag_mode == FMCW_MAG_AMBM;
    float* mrow = mags + rr * REGM;
#pragma unroll
    for (int g = 0; g < LG; ++g) {
      float* m0 = mrow + midx(t + P * g);
#pragma unroll
      for (int m = 0; m < LR; ++m)
        m0[mpadoff(m * (NC / LR))] = ambm ? acc[g][m] : mag_sqrt(acc[g][m]);
    }
    pass_sync<false>();
    if (cf.enabled) {
      fill_halo<NC, P>(mrow, t);
      pass_sync<false>();
    }

    // map store: WR*NC = 1024 floats contiguous at [f][r0][0], 16 B per lane
    {
      constexpr int Q = WR * NC / 4 / 64;
      const size_t mbase = ((size_t)f * ns + r0) * NC;
      const int lane = opaque(lane0);
#pragma unroll
      for (int i = 0; i < Q; ++i) {
        const int e = 4 * (lane + 64 * i);
        const int rl = e / NC, d = e - rl * NC;
        const float4 v = *reinterpret_cast<const float4*>(mags + rl * REGM + midx(d));
        if (lin_map) {
          st_f4<kNtMap>(lin_map + mbase + e, v);
        }
        if (!FAST && db_map) {
          const float k = 6.0205999132796239f;  // 20 / log2(10)
          *reinterpret_cast<float4*>(db_map + mbase + e) =
              make_float4(k * __log2f(v.x + 1.f), k * __log2f(v.y + 1.f), k * __log2f(v.z + 1.f),
                          k * __log2f(v.w + 1.f));
        }
      }
    }
    if (cf.enabled) {
      if constexpr (FAST)
        cfar1d_wave<NC, 8, 2, true>(mags, list, rr, t, r0, frame0 + f, tile0 + f * tiles_per_frame + lt, cf, sink);
      else
        cfar1d_dispatch<NC>(mags, list, rr, t, r0, frame0 + f, tile0 + f * tiles_per_frame + lt, cf, sink);
    }
    pass_sync<false>();  // the region is reused by the next tile
  }
  if constexpr (!FAST) {
    if (mti_rtl || q15d) {  // uniform
      status_add(status, n_wsat);
      status_add(status ? status + 1 : nullptr, n_msat);
    }
  }
}

}  // namespace fmcw
