// mimo_kernel.hpp -- k_mimo: the TDM-MIMO virtual array.  Splits the chirps of fmcw_range_ct's spectrum
// by transmitter and delays TX t's sequence by t / n_tx samples, so that all n_tx * n_rx virtual
// channels are sampled at TX 0's instants.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fft_device.hpp"

namespace fmcw {

// --------------------------------------------------------------------------------------
// Input   spec[f][k][r][c], c = m n_tx + t: one flat array of rows (f, k, r) of NC = n_tx ND points.
// Output  out[f][t n_rx + k][r][m], m < ND: the layout of a spectrum for (n_range, ND, n_tx n_rx).
//
// Wave tiles, as k_beams has them: ONE WAVEFRONT per tile of kMimoTile = 1024 consecutive input points
// = 1024 / NC whole rows of one (f, k) (n_range >= 64 rows, NC >= 32), which are S = 64 / P = 1024 / ND
// sequences u_t of ND points, P = ND / 16 lanes and 16 points a lane each; 4 independent waves per
// workgroup striding over the tiles of a capped grid, no workgroup barrier anywhere.  Lane l belongs to
// sequence s = l / P = (row of the tile) n_tx + t in every tile, so its transmitter and its 16 ramp
// factors are fixed for the launch.
//
// Per tile:
//   load      8 x 16 B per lane, consecutive lanes consecutive addresses: 1 KiB per instruction;
//   split     point c of a row -> sequence t = c mod n_tx, sample m = c / n_tx, in the wave's LDS
//             region (padded rows of the Stockham passes);
//   ALIGN_DFT the forward passes of fft_device.hpp in LDS (natural order out); then, per lane,
//             U[q] (rmp[q] / ND) with rmp[q] = exp(-2 pi i s(q) t / (n_tx ND)), q = t0 + P m, conjugated,
//             the first radix-16 pass from registers and the remaining passes in LDS: the forward
//             transform of the conjugate, whose conjugate is the inverse transform;
//   store     8 x 16 B per lane in output order [t][row][m]: the rows of one transmitter are
//             contiguous, 8 KiB / n_tx per tile, at least one 256-B output row.
// ALIGN_NONE is the instantiation without the transforms: moves only, so the copy is byte-exact.
// --------------------------------------------------------------------------------------
constexpr int kMimoTile = 1024;   // points per wave tile
constexpr int kMimoWPB = 4;       // waves per workgroup
constexpr int kMimoNT = 64 * kMimoWPB;

constexpr int mimo_log2(int n) { return n <= 1 ? 0 : 1 + mimo_log2(n / 2); }

template <int ND> struct MimoGeom {
  static constexpr int LG = mimo_log2(ND);
  static constexpr int P = ND / 16;                 // lanes per sequence
  static constexpr int S = 64 / P;                  // sequences per wave tile
  static constexpr int REG = padded(ND) + 4;        // complex per sequence row
  static constexpr int WCX = S * REG;               // complex per wave region
  static_assert(P >= 2 && P <= 64 && S * ND == kMimoTile, "32 <= ND <= 1024, a power of two");
};

// n_tx = 1 << lg_tx; n_range = 1 << lg_nr; n_tiles tiles of kMimoTile input points.
template <int ND, bool DFT>
__global__ void __launch_bounds__(kMimoNT)
k_mimo(const float2* __restrict__ spec, float2* __restrict__ out, int lg_tx, int n_rx, int lg_nr, int n_tiles) {
  using Gm = MimoGeom<ND>;
  constexpr int P = Gm::P, REG = Gm::REG, WCX = Gm::WCX, LG = Gm::LG;
  __shared__ __attribute__((aligned(16))) float2 lds[kMimoWPB * WCX];

  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane0 = threadIdx.x & 63;
  float2* const wreg = lds + wv * WCX;
  const int n_tx = 1 << lg_tx;
  const int lg_nc = lg_tx + LG;             // NC = n_tx ND <= 1024
  const int lg_chunk = 10 - lg_tx;          // output points of one transmitter per tile

  // the ramp of this lane's transmitter at its 16 bins, with the inverse transform's 1 / ND
  float2 rmp[16];
  if constexpr (DFT) {
    const int tx = (lane0 / P) & (n_tx - 1);
    const float per_rev = 1.0f / (float)(n_tx * ND), scale = 1.0f / ND;   // powers of two: exact
#pragma unroll
    for (int m = 0; m < 16; ++m) {
      const int q = lane0 % P + P * m;
      const int sq = q < ND / 2 ? q : q - ND;             // the Nyquist bin takes the negative sign
      const float rev = -(float)(sq * tx) * per_rev;      // |rev| < 1/2, exact
      // v_cos / v_sin take revolutions; the products below, not an asm reader, consume their results
      rmp[m] = make_float2(__builtin_amdgcn_cosf(rev) * scale, __builtin_amdgcn_sinf(rev) * scale);
    }
  }

  for (int tile = (int)blockIdx.x * kMimoWPB + wv; tile < n_tiles; tile += (int)gridDim.x * kMimoWPB) {
    const int lane = opaque(lane0);
    {  // load and split
      const float2* const in = spec + (size_t)tile * kMimoTile;
      float4 x[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) x[i] = ld_f4<kNtSpecLd>(in + 2 * (lane + 64 * i));
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int p = 2 * (lane + 64 * i);                // points p, p + 1 of the tile: one row (NC is even)
        const int row = p >> lg_nc, c = p & ((1 << lg_nc) - 1);
        float2* const rows = wreg + (row << lg_tx) * REG;
        rows[(c & (n_tx - 1)) * REG + pad16(c >> lg_tx)] = make_float2(x[i].x, x[i].y);
        rows[((c + 1) & (n_tx - 1)) * REG + pad16((c + 1) >> lg_tx)] = make_float2(x[i].z, x[i].w);
      }
    }
    pass_sync<false>();
    if constexpr (DFT) {
      const int t = lane % P;
      float2* const buf = wreg + (lane / P) * REG;
      stockham_from<ND, 1, P, false>(buf, t);             // U[q], natural order
      float2 v[16];
      {
        const float2* src = buf + pad16(t);
#pragma unroll
        for (int m = 0; m < 16; ++m) v[m] = src[padoff(m * P)];
      }
      pass_sync<false>();
#pragma unroll
      for (int m = 0; m < 16; ++m) {
        v[m] = cmul(v[m], rmp[m]);
        v[m].y = -v[m].y;
      }
      Dft<16>::run(v);                                    // pass 1 of the transform of the conjugate: L = 1
      {
        float2* d = buf + pad16(16 * t);                  // y[16 t + m]
#pragma unroll
        for (int m = 0; m < 16; ++m) d[m] = v[m];
      }
      pass_sync<false>();
      stockham_from<ND, 16, P, false>(buf, t);
    }
    {  // store: [t][row][m] of the tile, 16 B per lane
      const uint32_t row0 = (uint32_t)tile << (10 - lg_nc);             // the tile's first row (f, k, r)
      const uint32_t fk = row0 >> lg_nr, r0 = row0 & ((1u << lg_nr) - 1u);
      const uint32_t f = fk / (uint32_t)n_rx, k = fk - f * (uint32_t)n_rx;
      const size_t v0 = (size_t)f * n_tx * n_rx + k;                    // virtual channel of TX 0
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int p = 2 * (lane + 64 * i);
        const int tx = p >> lg_chunk, rem = p & ((1 << lg_chunk) - 1);
        const int row = rem >> LG, m = rem & (ND - 1);
        const float2* src = wreg + ((row << lg_tx) + tx) * REG + pad16(m);   // m even: m + 1 is the next slot
        float2 a = src[0], b = src[1];
        if constexpr (DFT) {
          a.y = -a.y;
          b.y = -b.y;
        }
        const size_t orow = ((v0 + (size_t)tx * n_rx) << lg_nr) + r0 + row;
        st_f4<kNtSpecSt>(out + orow * ND + m, make_float4(a.x, a.y, b.x, b.y));
      }
    }
    pass_sync<false>();   // the region is rewritten by the next tile
  }
}

}  // namespace fmcw
