// cacfar_kernel.hpp -- k_cacfar / k_cacfar_scan: the cell-averaging CFAR (CA / GO / SO) of
// include/fmcw.h "Cell-averaging CFAR", a count pass, a scan and an emit pass.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "det_sink.hpp"
#include "fft_device.hpp"

namespace fmcw {

// --------------------------------------------------------------------------------------
// Geometry.  A tile is a strip of `strip` range rows of one frame, all Doppler bins; tiles are
// numbered in (frame, range) order, so the tiles' detection runs, each in (range, doppler) order,
// concatenate to the ordered list.  Persistent workgroups of 256 threads stride over the tiles.
//
// A strip walks down in range, `rps` = max(1, 1024 / n_doppler) rows per step (1024 cells: thread
// tid owns the 4 cells (j, d0 .. d0+3), j = 4 tid / n_doppler, of the step's row group, which is
// also the list order).  Per step and thread, for the step's first new row r0 (its CUT rows end at
// r0 + rps - 1 - Hr):
//   (a) 16-byte loads of row rn = r0 + j (for H), of row rn - Rr (its Lg completes the window of
//       CUT row rn - Hr) and of the CUT row rn - Hr itself (kept in registers); the first two go to
//       two LDS staging row groups, clamped (nonneg).  The second and third rows were read Rr and Hr
//       rows ago by this workgroup: they come from L2.  The loads are issued one step ahead.
//   (b) Lg, Cg, Rg and H = (Lg + Cg) + Rg of the 4 cells of rn from the staged row, the Doppler
//       wrap inside the row; H goes to the H ring (2 Hr + rps rows), Lg of row rn - Rr to the Lg ring
//       (2 Gr + rps rows).  No Rg ring: Rg[r][d] = Lg[r][d + Hd + Gd + 1], the same terms in the same
//       order, so R reads the Lg ring shifted.
//   (c) the decision of CUT row rn - Hr: U, D over the H ring, L, R over the Lg ring, each in the
//       canonical ascending order from its first term (accumulators start at +0, which is exact:
//       every term is >= +0).
// The rings hold rows by (row mod ring size).  Two barriers per step: after the staging stores and
// after the ring stores; the next step's staging stores come after the second, its ring stores
// after its own first, so no step overwrites what another thread still reads.
//
// k_cacfar<false, *> counts a tile's detections into counts[tile]; k_cacfar_scan turns the counts into
// exclusive offsets and writes the status words; k_cacfar<true, *> repeats the same arithmetic on the
// same map and stores the records at offs[tile] + (rank inside the tile), below det_cap only.
// --------------------------------------------------------------------------------------
constexpr int kCaNT = 256;          // threads per workgroup
constexpr int kCaStepCells = 1024;  // cells per step: 4 per thread

struct CaCfarArgs {
  int ns, lg_nd;        // range rows; log2(n_doppler)
  int mode;             // fmcw_cacfar_mode
  int rr, gr, rd, gd;   // reference and guard extents, range / Doppler
  float k;              // kc (CA) or kh (GO, SO): formed once on the host
  int rps;              // rows per step
  int strip;            // range rows per tile
  int tiles_per_frame;
};

// floats of the workgroup's dynamic LDS: H ring, Lg ring, two staging row groups
__host__ __device__ inline size_t cacfar_lds_floats(int nd, int hr, int gr, int rps) {
  return (size_t)((2 * hr + rps) + (2 * gr + rps) + 2 * rps) * (size_t)nd;
}

// sum of row[(d + dd) & mask] for dd = lo .. hi in ascending order (+0 when empty)
__device__ __forceinline__ float ca_seg(const float* row, int d, int lo, int hi, int mask) {
  float s = 0.f;
  for (int dd = lo; dd <= hi; ++dd) s += row[(d + dd) & mask];
  return s;
}

// DEF: the default window 4/1/4/2 as compile-time constants, so that every window loop unrolls, the
// LDS reads of a sum are issued together and the 4 cells of a thread share the reads of their common
// span; the other windows run the same code with the extents read from `g`.
template <bool EMIT, bool DEF>
__global__ void __launch_bounds__(kCaNT)
k_cacfar(const float* __restrict__ map, CaCfarArgs g, int n_tiles, uint32_t* __restrict__ counts,
         const uint32_t* __restrict__ offs, fmcw_det* __restrict__ dets, uint32_t det_cap) {
  extern __shared__ __attribute__((aligned(16))) float ca_lds[];
  __shared__ int s_wave[kCaNT / 64];
  const int nd = 1 << g.lg_nd, mask = nd - 1;
  const int rps = g.rps;
  const int w_rr = DEF ? 4 : g.rr, w_gr = DEF ? 1 : g.gr, w_rd = DEF ? 4 : g.rd, w_gd = DEF ? 2 : g.gd;
  const int hr = w_rr + w_gr, hd = w_rd + w_gd;
  const int ring_h = 2 * hr + rps, ring_l = 2 * w_gr + rps;
  float* const hring = ca_lds;
  float* const lring = hring + ring_h * nd;
  float* const st_h = lring + ring_l * nd;   // the step's new rows
  float* const st_l = st_h + rps * nd;       // the rows Rr behind them
  const int tid = threadIdx.x;
  const int j = (4 * tid) >> g.lg_nd;
  const int d0 = (4 * tid) & mask;
  const int r_shift = hd + w_gd + 1;         // Rg[d] = Lg[d + r_shift]

  for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int f = tile / g.tiles_per_frame;
    const int ts = tile - f * g.tiles_per_frame;
    const int c0 = max(ts * g.strip, hr), c1 = min((ts + 1) * g.strip, g.ns - hr);   // the tile's CUT rows
    const float* const fmap = map + (size_t)f * g.ns * nd;
    uint32_t run = 0;   // records of this tile before the current step (uniform)
    if constexpr (EMIT) run = offs[tile];
    int mine = 0;       // this thread's detections in the tile (count pass)

    // the three rows of a step, raw (clamped where they are used, so that nothing waits on them here)
    auto load_step = [&](int r0, float4& vn, float4& vl, float4& vc) {
      const int rn = r0 + j, rl = rn - w_rr, rc = rn - hr;
      vn = vl = vc = make_float4(0.f, 0.f, 0.f, 0.f);
      if (rn < g.ns) vn = ld_f4<false>(fmap + (size_t)rn * nd + d0);
      if (rl >= 0 && rl < g.ns) vl = ld_f4<false>(fmap + (size_t)rl * nd + d0);
      if (rc >= c0 && rc < c1) vc = ld_f4<false>(fmap + (size_t)rc * nd + d0);
    };
    float4 pn, pl, pc;
    load_step(c0 - hr, pn, pl, pc);

    for (int r0 = c0 - hr; r0 - hr < c1; r0 += rps) {
      const int rn = r0 + j, rl = rn - w_rr, rc = rn - hr;
      const bool new_ok = rn < g.ns, l_ok = rl >= 0 && rl < g.ns, cut = rc >= c0 && rc < c1;
      // (a): this step's rows were loaded a step ago; the next step's loads stay in flight over (b), (c)
      *reinterpret_cast<float4*>(st_h + j * nd + d0) = nonneg4(pn);
      *reinterpret_cast<float4*>(st_l + j * nd + d0) = nonneg4(pl);
      const float4 vc = nonneg4(pc);
      if (r0 + rps - hr < c1) load_step(r0 + rps, pn, pl, pc);
      __syncthreads();
      // (b)
      if (new_ok) {
        const float* row = st_h + j * nd;
        float h[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const float lg = ca_seg(row, d0 + c, -hd, -w_gd - 1, mask);
          const float cg = ca_seg(row, d0 + c, -w_gd, w_gd, mask);
          const float rg = ca_seg(row, d0 + c, w_gd + 1, hd, mask);
          h[c] = (lg + cg) + rg;
        }
        *reinterpret_cast<float4*>(hring + (rn % ring_h) * nd + d0) = make_float4(h[0], h[1], h[2], h[3]);
      }
      if (l_ok) {
        const float* row = st_l + j * nd;
        float l[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) l[c] = ca_seg(row, d0 + c, -hd, -w_gd - 1, mask);
        *reinterpret_cast<float4*>(lring + (rl % ring_l) * nd + d0) = make_float4(l[0], l[1], l[2], l[3]);
      }
      __syncthreads();
      // (c)
      uint32_t flags = 0;
      float thr[4] = {0.f, 0.f, 0.f, 0.f};
      if (cut) {
        float u[4] = {0.f, 0.f, 0.f, 0.f}, dn[4] = {0.f, 0.f, 0.f, 0.f};
        float lsum[4] = {0.f, 0.f, 0.f, 0.f}, rsum[4] = {0.f, 0.f, 0.f, 0.f};
        int slot = (rc - hr) % ring_h;
        for (int i = 0; i < w_rr; ++i) {               // dr = -Hr .. -Gr-1
          const float4 v = *reinterpret_cast<const float4*>(hring + slot * nd + d0);
          u[0] += v.x; u[1] += v.y; u[2] += v.z; u[3] += v.w;
          slot = slot + 1 == ring_h ? 0 : slot + 1;
        }
        slot += 2 * w_gr + 1;                          // the guard rows
        if (slot >= ring_h) slot -= ring_h;
        for (int i = 0; i < w_rr; ++i) {               // dr = Gr+1 .. Hr
          const float4 v = *reinterpret_cast<const float4*>(hring + slot * nd + d0);
          dn[0] += v.x; dn[1] += v.y; dn[2] += v.z; dn[3] += v.w;
          slot = slot + 1 == ring_h ? 0 : slot + 1;
        }
        slot = (rc - w_gr) % ring_l;
        for (int i = 0; i < 2 * w_gr + 1; ++i) {       // dr = -Gr .. Gr
          const float* row = lring + slot * nd;
          const float4 v = *reinterpret_cast<const float4*>(row + d0);
          lsum[0] += v.x; lsum[1] += v.y; lsum[2] += v.z; lsum[3] += v.w;
#pragma unroll
          for (int c = 0; c < 4; ++c) rsum[c] += row[(d0 + c + r_shift) & mask];
          slot = slot + 1 == ring_l ? 0 : slot + 1;
        }
        const float m[4] = {vc.x, vc.y, vc.z, vc.w};
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const float a = u[c] + lsum[c], b = dn[c] + rsum[c];
          // One multiplication of a sum, a maximum or a minimum: nothing here (or above: adds
          // only) is a multiply followed by an add, and there is no division, so no contraction
          // or reciprocal can change a bit.
          const float s = g.mode == FMCW_CACFAR_CA ? a + b : g.mode == FMCW_CACFAR_GO ? fmaxf(a, b) : fminf(a, b);
          thr[c] = g.k * s;
          flags |= (m[c] > thr[c] ? 1u : 0u) << c;
        }
      }
      const int n = __popc(flags);
      if constexpr (EMIT) {
        int total;
        uint32_t idx = run + (uint32_t)block_excl_scan1<kCaNT>(n, s_wave, total);
        run += (uint32_t)total;
        const float m[4] = {vc.x, vc.y, vc.z, vc.w};
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          if (flags >> c & 1u) {
            if (idx < det_cap) {
              const fmcw_u4v rec = {(uint32_t)f, (uint32_t)rc | (uint32_t)(d0 + c) << 16, __float_as_uint(m[c]),
                                    __float_as_uint(thr[c])};
              *reinterpret_cast<fmcw_u4v*>(dets + idx) = rec;
            }
            ++idx;
          }
        }
      } else {
        mine += n;
      }
    }
    if constexpr (!EMIT) {
      int total;
      block_excl_scan1<kCaNT>(mine, s_wave, total);
      if (tid == 0) counts[tile] = (uint32_t)total;
    }
  }
}

// One workgroup: offs[i] = counts[0] + .. + counts[i-1]; status = {the sum, 0, 0, 0}.  With
// n_tiles == 0 it writes the four words only.
constexpr int kCaScanNT = 1024;
__global__ void __launch_bounds__(kCaScanNT)
k_cacfar_scan(const uint32_t* __restrict__ counts, uint32_t* __restrict__ offs, int n_tiles,
              uint32_t* __restrict__ status) {
  const uint32_t sum = tile_offsets_scan<kCaScanNT>(counts, offs, n_tiles);   // a tile has at most 2^16 cells
  if (threadIdx.x < FMCW_STATUS_WORDS) status[threadIdx.x] = threadIdx.x == 0 ? sum : 0u;
}

}  // namespace fmcw
