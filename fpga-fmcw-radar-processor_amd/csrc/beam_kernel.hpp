// beam_kernel.hpp -- k_beams: weights over rx + MTI + Doppler window + FFT + |X|, one map per beam.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cfar1d.hpp"
#include "fft_device.hpp"
#include "spec_rows.hpp"

namespace fmcw {

// --------------------------------------------------------------------------------------
// Coherent beamforming between fmcw_range_ct and fmcw_cfar: K2's sibling.  Where k_doppler sums
// |X_rx|^2 over the channels after the transform, k_beams sums W[b][k] x_k before it and
// transforms once per beam, so the channels add in phase.
//
// The geometry is DopplerGeom<NC>'s (cfar1d.hpp "Wave tiles"): lane (rr, t) of P = NC/16 owns range
// row r0 + rr's 16 chirps c = t + P m, one wavefront per tile of WR = 64/P rows, 4 independent
// waves per workgroup striding over the tiles of a capped grid; no workgroup barrier anywhere.
// The input is fmcw_range_ct's plain [frame][rx][range][chirp] spectrum: the WR rows of one
// channel are one contiguous WR * NC * 8 = 8 KiB block, which the 16 loads of a wave cover whole.
//
// Per tile and beam (the streaming form: every beam re-reads the channels' points, from L1 / L2
// after the first, and the registers do not grow with n_rx):
//   v[m] = sum_k W[b][k] y_k[m], k = 0 .. n_rx-1 in that order (four fmaf per term: the result
//   depends on the inputs alone, not on the grid or the wave); y_k the canceller over x_k
//   (spec_rows.hpp's mti_point: its neighbours x[c-1], x[c-2] loaded directly, the lines the
//   neighbouring lanes just asked for);
//   W[b][k] is uniform and arrives through the scalar cache;
//   v[m] *= w[c]; Dft<16>; the LDS rows; the remaining passes with the last one in registers;
//   |X| -> the wave's LDS region -> 16 B per lane, non-temporal, to maps[f][b][r0..][0..].
// --------------------------------------------------------------------------------------
// floats of a wave's LDS region: the two FFT row sets, later the magnitude rows (no cell list)
template <int NC> constexpr int beam_wave_floats() {
  using Gm = DopplerGeom<NC>;
  return cmax(2 * Gm::WR * Gm::REGD, Gm::WR * Gm::REGM);
}

template <int NC, int MTI>
__global__ void __launch_bounds__(DopplerGeom<NC>::NT)
k_beams(const float2* __restrict__ spec, const float2* __restrict__ wts, const float* __restrict__ win_d, int ns,
        int nrx, int nb, int n_tiles, float* __restrict__ maps) {
  using Gm = DopplerGeom<NC>;
  constexpr int P = Gm::P, WR = Gm::WR, WPB = Gm::WPB, REGD = Gm::REGD, REGM = Gm::REGM;
  constexpr int LR = Gm::LR, LG = Gm::LG;
  constexpr int WFL = beam_wave_floats<NC>();
  static_assert(P <= 64 && WFL % 4 == 0, "a Doppler transform fits one wave; 16-B aligned regions");
  __shared__ __attribute__((aligned(16))) float lds[WPB * WFL];

  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane0 = threadIdx.x & 63;
  const int rr = lane0 / P;
  const int t0 = lane0 % P;
  float* const mags = lds + wv * WFL;
  float2* const wreg = reinterpret_cast<float2*>(mags);
  const int tiles_per_frame = ns / WR;
  const size_t rx_step = (size_t)ns * NC;
  // the Doppler window of this lane's chirps (ones for FMCW_WIN_NONE)
  float wv_d[16];
#pragma unroll
  for (int m = 0; m < 16; ++m) wv_d[m] = win_d[t0 + P * m];
  // last-pass twiddle bases, once per lane, where K2 keeps them (NC = 256)
  constexpr bool TWH = NC / 16 <= 16 && P % 16 == 0;
  GroupTwiddles<NC / 16, NC> twh;
  if constexpr (TWH) twh.init(t0 & 15);

  for (int tile = (int)blockIdx.x * WPB + wv; tile < n_tiles; tile += (int)gridDim.x * WPB) {
    const int f = tile / tiles_per_frame;
    const int r0 = (tile - f * tiles_per_frame) * WR;
    const float2* const row0 = spec + (size_t)f * nrx * rx_step + (size_t)(r0 + rr) * NC;  // channel 0
    for (int b = 0; b < nb; ++b) {
      const int t = opaque(t0);
      float2* buf = wreg + rr * REGD;
      float2 v[16];
#pragma unroll
      for (int m = 0; m < 16; ++m) v[m] = make_float2(0.f, 0.f);
      const float2* src = row0;
      for (int k = 0; k < nrx; ++k, src += rx_step) {
        const float2 w = wts[b * nrx + k];  // uniform
#pragma unroll
        for (int m = 0; m < 16; ++m) {
          const int c = t + P * m;
          const float2 x = mti_point<MTI>(src + c, (uint32_t)c);
          v[m].x = fmaf(-w.y, x.y, fmaf(w.x, x.x, v[m].x));
          v[m].y = fmaf(w.y, x.x, fmaf(w.x, x.y, v[m].y));
        }
      }
#pragma unroll
      for (int m = 0; m < 16; ++m) v[m] = cscale(v[m], wv_d[m]);
      Dft<16>::run(v);                       // pass 1: L = 1, no twiddles
      {
        float2* d = buf + pad16(16 * t);     // y[16 t + m]
#pragma unroll
        for (int m = 0; m < 16; ++m) d[m] = v[m];
      }
      pass_sync<false>();
      float2 X[LG][LR];
      if constexpr (TWH) stockham_last_tw<NC, 16, P>(buf, t, X, twh);
      else stockham_to_regs<NC, 16, P, false>(buf, t, X);
      pass_sync<false>();  // every read of the last pass is issued: the rows may be rewritten
      // magnitudes -> the wave region (over the dead FFT rows), for the map store
      float* mrow = mags + rr * REGM;
#pragma unroll
      for (int g = 0; g < LG; ++g) {
        float* m0 = mrow + midx(t + P * g);
#pragma unroll
        for (int m = 0; m < LR; ++m) m0[mpadoff(m * (NC / LR))] = mag_sqrt(cabs2(X[g][m]));
      }
      pass_sync<false>();
      // map store: WR * NC = 1024 floats contiguous at [f][b][r0][0], 16 B per lane
      {
        constexpr int Q = WR * NC / 4 / 64;
        const size_t mbase = (((size_t)f * nb + b) * ns + r0) * NC;
        const int lane = opaque(lane0);
#pragma unroll
        for (int i = 0; i < Q; ++i) {
          const int e = 4 * (lane + 64 * i);
          const int rl = e / NC, d = e - rl * NC;
          st_f4<kNtMap>(maps + mbase + e, *reinterpret_cast<const float4*>(mags + rl * REGM + midx(d)));
        }
      }
      pass_sync<false>();  // the region is reused by the next beam
    }
  }
}

}  // namespace fmcw
