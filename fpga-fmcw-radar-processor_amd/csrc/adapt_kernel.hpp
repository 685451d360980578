// adapt_kernel.hpp -- k_adapt_acc, k_adapt_solve: the sample covariance of the rx channels over the
// training cells and the loaded minimum-variance (MVDR) solve for the beamformer's weights.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/fmcw.h"
#include "spec_rows.hpp"

namespace fmcw {

// --------------------------------------------------------------------------------------
// Stage 1, k_adapt_acc: R = (1/K) sum z z^H as a real Gram matrix on the matrix cores.
//
// With y = [Re z_0 .. Re z_{NP-1}, Im z_0 .. Im z_{NP-1}] (ROWS = 2 NP real rows, the rows of the
// channels beyond n_rx zero) the ROWS x ROWS matrix G = sum y y^T holds every product R needs:
//   Re R[i][j] = G[i][j] + G[NP+i][NP+j],   Im R[i][j] = G[NP+i][j] - G[i][NP+j].
// One f32 MFMA adds KK = 64 / ROWS snapshots to the whole tile: the A operand of lane l is
// y[l % ROWS] of snapshot l / ROWS, and B is A's transpose, the same register.  Two tiles:
//   ROWS 32: v_mfma_f32_32x32x2_f32, 16 accumulator VGPRs, n_rx 9 .. 16
//   ROWS 16: v_mfma_f32_16x16x4_f32,  4 accumulator VGPRs, n_rx 1 .. 8 (4 snapshots per 32 cycles
//            where the 32-row tile takes 2 per 64)
//
// The training window [train_r0, train_r0 + train_rows) of one (frame, rx) plane of
// [frame][rx][range][chirp] is ONE contiguous run of Cf = train_rows * n_doppler points.  A step is
// 64 consecutive points of that run in every channel: lane s loads point 64 sb + s of channel k,
// 512 contiguous bytes per wave and channel (with MTI, spec_rows.hpp's mti_point, also its two
// predecessors in the row, the lines the neighbouring lanes ask for), and writes the two real rows to the wave's LDS tile
// [snapshot][ROWS + 1]; the ROWS MFMAs of the step read their operand back transposed, lane l from
// [KK m + l / ROWS][l % ROWS].  Both the stride-(ROWS+1) write and the contiguous read are free of
// bank conflicts.  A lane past Cf (the last step of a frame) writes zeros.  There is no branch
// around the loads, so a step's loads of all channels are in flight together.
//
// Units: the T = n_frames * ceil(Cf / 64) steps of a call are split into n_units = min(T,
// kAdaptMaxUnits) contiguous runs, unit u = steps [u T / n_units, (u+1) T / n_units): a function
// of the shape and n_frames alone.  One wave sums one unit in its accumulator tile and stores the
// whole tile to part[u][ROWS][ROWS]; the waves of a capped grid stride over the units.  No atomics;
// which wave takes a unit changes nothing.  Every word of part[0 .. n_units) is written by the
// launch that the solve of the same call reads.
// --------------------------------------------------------------------------------------
constexpr int kAdaptMaxUnits = 2048;
constexpr int kAdaptThreads = 256;            // 4 waves, one unit each at a time
constexpr int kAdaptWaves = kAdaptThreads / 64;

struct AdaptGeom {
  uint32_t nd;            // n_doppler
  uint32_t nrx;
  uint32_t cf;            // training points per (frame, rx) plane
  uint32_t spf;           // steps per frame, ceil(cf / 64)
  uint32_t n_steps;       // T
  uint32_t n_units;
  uint32_t off0;          // train_r0 * n_doppler
  uint32_t rx_step;       // n_range * n_doppler
};

typedef float adapt_f16v __attribute__((ext_vector_type(16)));
typedef float adapt_f4v __attribute__((ext_vector_type(4)));

template <int ROWS> struct AdaptTile;
template <> struct AdaptTile<32> {
  using Acc = adapt_f16v;
  static constexpr int NV = 16;
  static __device__ __forceinline__ Acc mma(float a, Acc c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, a, c, 0, 0, 0); }
  // accumulator register v of lane l: row, column
  static __device__ __forceinline__ int row(int l, int v) { return (v & 3) + 8 * (v >> 2) + 4 * (l >> 5); }
};
template <> struct AdaptTile<16> {
  using Acc = adapt_f4v;
  static constexpr int NV = 4;
  static __device__ __forceinline__ Acc mma(float a, Acc c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, a, c, 0, 0, 0); }
  static __device__ __forceinline__ int row(int l, int v) { return 4 * (l >> 4) + v; }
};

template <int ROWS, int MTI>
__global__ void __launch_bounds__(kAdaptThreads)
k_adapt_acc(const float2* __restrict__ spec, AdaptGeom g, float* __restrict__ part) {
  using Tile = AdaptTile<ROWS>;
  constexpr int NP = ROWS / 2, LD = ROWS + 1, KK = 64 / ROWS;
  __shared__ float lds[kAdaptWaves * 64 * LD];
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  float* const tile = lds + wv * 64 * LD;
  float* const mine = tile + lane * LD;                            // this lane's snapshot: ROWS rows
  const float* const opnd = tile + (lane / ROWS) * LD + lane % ROWS;   // + KK * LD per MFMA
  // the rows of the channels beyond n_rx stay zero for the whole launch
  for (int i = 0; i < ROWS; ++i) mine[i] = 0.f;
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");

  for (uint32_t u = blockIdx.x * kAdaptWaves + wv; u < g.n_units; u += gridDim.x * kAdaptWaves) {
    const uint32_t s0 = (uint32_t)((uint64_t)u * g.n_steps / g.n_units);
    const uint32_t s1 = (uint32_t)((uint64_t)(u + 1) * g.n_steps / g.n_units);
    typename Tile::Acc acc;
#pragma unroll
    for (int v = 0; v < Tile::NV; ++v) acc[v] = 0.f;
    for (uint32_t s = s0; s < s1; ++s) {
      const uint32_t f = s / g.spf;
      const uint32_t e = (s - f * g.spf) * 64 + lane;   // the point of the frame's training run
      const bool live = e < g.cf;
      const uint32_t ec = live ? e : 0u;                // a lane past the run loads point 0 and drops it
      const uint32_t c = ec & (g.nd - 1);               // its chirp
      // no branch around the loads (mti_point's neither): the channels' loads of a step are in
      // flight together
      const float2* src = spec + (size_t)f * g.nrx * g.rx_step + g.off0 + ec;
#pragma unroll 8
      for (uint32_t k = 0; k < g.nrx; ++k, src += g.rx_step) {
        const float2 x = mti_point<MTI>(src, c);
        mine[k] = live ? x.x : 0.f;
        mine[NP + k] = live ? x.y : 0.f;
      }
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
#pragma unroll 8
      for (int m = 0; m < ROWS; ++m) acc = Tile::mma(opnd[m * KK * LD], acc);
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");   // the tile may be rewritten
    }
    float* const dst = part + (size_t)u * (ROWS * ROWS) + lane % ROWS;
#pragma unroll
    for (int v = 0; v < Tile::NV; ++v) dst[Tile::row(lane, v) * ROWS] = acc[v];
  }
}

// --------------------------------------------------------------------------------------
// Stage 2 in fp64, two launches: k_adapt_fold, then k_adapt_solve.
//
// k_adapt_fold: the units' tiles summed in fp64 into n_parts = min(n_units, kAdaptFoldParts) tiles,
// workgroup g the units [g n_units / n_parts, (g+1) n_units / n_parts) in ascending order, one
// thread per entry.  It exists for time alone: 2048 tiles of 4 KiB read by the one workgroup of the
// solve cost 20 us (n_rx 4) to 85 us (n_rx 16) of a call; spread over 64 workgroups it is a few us.
// The grouping is a function of n_units alone, so the sum's order is as fixed as before.
//
// k_adapt_solve: one workgroup of 1024 threads.
//   1. G[e] = sum over the parts of part2[g][e] in ascending g.  With the 16-row tile four threads
//      share an entry (contiguous quarters of the parts), combined in ascending order.
//   2. R from G's lower triangle (the upper one is its conjugate, the diagonal real), cov, delta.
//   3. Cholesky Rl = L L^H, left-looking, thread i owning row i; a pivot that is not above
//      FMCW_ADAPT_PIVOT_MIN times the mean diagonal of Rl (NaN included) ends it with the
//      fallback flag.
//   4. thread b: L y = a_b, L^H x = y, den = y^H y, W[b][k] = conj(x_k) / den; a beam whose
//      weights are not finite falls back as well.
// --------------------------------------------------------------------------------------
constexpr int kSolveThreads = 1024;
constexpr int kAdaptFoldParts = 64;

__global__ void __launch_bounds__(256)
k_adapt_fold(const float* __restrict__ part, uint32_t n_units, uint32_t n_parts, uint32_t E, double* __restrict__ part2) {
  const uint32_t g = blockIdx.x;
  const uint32_t u0 = (uint32_t)((uint64_t)g * n_units / n_parts), u1 = (uint32_t)((uint64_t)(g + 1) * n_units / n_parts);
  for (uint32_t e = threadIdx.x; e < E; e += 256) {
    const float* src = part + e;
    double s = 0.0;
#pragma unroll 8
    for (uint32_t u = u0; u < u1; ++u) s += (double)src[(size_t)u * E];
    part2[(size_t)g * E + e] = s;
  }
}

struct SolveArgs {
  uint32_t nrx, nb, rows, n_units, n_parts;
  uint64_t K;
  double loading;
};

__global__ void __launch_bounds__(kSolveThreads)
k_adapt_solve(const double* __restrict__ part2, const float2* __restrict__ a_dev, SolveArgs p, float2* __restrict__ w_out,
              double2* __restrict__ cov_out, uint32_t* __restrict__ info) {
  __shared__ double sG[kSolveThreads];
  __shared__ double2 sL[16 * 16];
  __shared__ double2 sY[64 * 16];
  __shared__ double sPiv;
  __shared__ int sFlags;
  const int t = threadIdx.x;
  const int n = (int)p.nrx, rows = (int)p.rows, np = rows / 2;
  const int E = rows * rows, P = kSolveThreads / E;
  if (t == 0) sFlags = 0;
  {
    const int e = t % E, q = t / E;
    const uint32_t u0 = (uint32_t)q * p.n_parts / P, u1 = (uint32_t)(q + 1) * p.n_parts / P;
    const double* src = part2 + e;
    double s = 0.0;
#pragma unroll 8
    for (uint32_t u = u0; u < u1; ++u) s += src[(size_t)u * E];
    sG[t] = s;
  }
  __syncthreads();
  const double invK = 1.0 / (double)p.K;
  if (t < n * n) {
    const int i = t / n, j = t % n;
    const int hi = i >= j ? i : j, lo = i >= j ? j : i;   // the lower-triangle entry (hi, lo)
    double rr = 0.0, ii = 0.0, ri = 0.0, ir = 0.0;
    for (int q = 0; q < P; ++q) {
      const double* G = sG + q * E;
      rr += G[hi * rows + lo];
      ii += G[(np + hi) * rows + np + lo];
      ir += G[(np + hi) * rows + lo];
      ri += G[(np + lo) * rows + hi];   // = G[hi][np + lo]: the tile is symmetric
    }
    double2 r = make_double2((rr + ii) * invK, hi == lo ? 0.0 : (ir - ri) * invK);
    if (i < j) r.y = -r.y;
    sL[i * 16 + j] = r;
    if (cov_out) cov_out[i * n + j] = r;
  }
  __syncthreads();
  if (t == 0) {
    double tr = 0.0;
    for (int i = 0; i < n; ++i) tr += sL[i * 16 + i].x;
    const double delta = p.loading * tr / (double)n;
    sPiv = FMCW_ADAPT_PIVOT_MIN * (tr / (double)n + delta);
    for (int i = 0; i < n; ++i) sL[i * 16 + i].x += delta;
    info[0] = (uint32_t)p.K;
    info[1] = (uint32_t)(p.K >> 32);
    info[3] = p.n_units;
    const uint64_t db = (uint64_t)__double_as_longlong(delta);
    info[4] = (uint32_t)db;
    info[5] = (uint32_t)(db >> 32);
    info[6] = info[7] = 0u;
  }
  __syncthreads();
  const double piv_min = sPiv;
  for (int j = 0; j < n; ++j) {
    // row i >= j: s = Rl[i][j] - sum_{k<j} L[i][k] conj(L[j][k]), in place
    if (t >= j && t < n) {
      double2 s = sL[t * 16 + j];
      for (int k = 0; k < j; ++k) {
        const double2 a = sL[t * 16 + k], b = sL[j * 16 + k];
        s.x -= a.x * b.x + a.y * b.y;
        s.y -= a.y * b.x - a.x * b.y;
      }
      sL[t * 16 + j] = s;
    }
    __syncthreads();
    const double piv = sL[j * 16 + j].x;
    if (!(piv > piv_min)) {   // uniform: every thread reads the same word
      if (t == 0) sFlags = FMCW_ADAPT_FALLBACK;
      break;
    }
    __syncthreads();   // the pivot is read before row j rewrites it
    if (t >= j && t < n) {
      const double d = 1.0 / sqrt(piv);
      double2 s = sL[t * 16 + j];
      sL[t * 16 + j] = t == j ? make_double2(sqrt(piv), 0.0) : make_double2(s.x * d, s.y * d);
    }
    __syncthreads();
  }
  __syncthreads();
  const bool fallback = sFlags != 0;
  if (t < (int)p.nb) {
    const float2* a = a_dev + (size_t)t * n;
    double2* y = sY + t * 16;
    double a2 = 0.0;
    for (int k = 0; k < n; ++k) a2 += (double)a[k].x * a[k].x + (double)a[k].y * a[k].y;
    bool conv = fallback;
    if (!conv) {
      double den = 0.0;
      for (int i = 0; i < n; ++i) {   // L y = a
        double2 s = make_double2((double)a[i].x, (double)a[i].y);
        for (int k = 0; k < i; ++k) {
          const double2 l = sL[i * 16 + k], v = y[k];
          s.x -= l.x * v.x - l.y * v.y;
          s.y -= l.x * v.y + l.y * v.x;
        }
        const double d = 1.0 / sL[i * 16 + i].x;
        y[i] = make_double2(s.x * d, s.y * d);
        den += y[i].x * y[i].x + y[i].y * y[i].y;
      }
      for (int i = n - 1; i >= 0; --i) {   // L^H x = y, in place
        double2 s = y[i];
        for (int k = i + 1; k < n; ++k) {
          const double2 l = sL[k * 16 + i], v = y[k];   // conj(L[k][i]) x[k]
          s.x -= l.x * v.x + l.y * v.y;
          s.y -= l.x * v.y - l.y * v.x;
        }
        const double d = 1.0 / sL[i * 16 + i].x;
        y[i] = make_double2(s.x * d, s.y * d);
      }
      const double inv = 1.0 / den;
      bool ok = den > 0.0 && isfinite(inv);
      for (int k = 0; k < n; ++k) {
        y[k] = make_double2(y[k].x * inv, -y[k].y * inv);
        ok = ok && isfinite((float)y[k].x) && isfinite((float)y[k].y);
      }
      if (!ok) {
        conv = true;
        atomicOr(&sFlags, (int)FMCW_ADAPT_FALLBACK);
      }
    }
    if (conv) {
      const double inv = 1.0 / a2;   // a_b != 0 (create)
      for (int k = 0; k < n; ++k) y[k] = make_double2((double)a[k].x * inv, -(double)a[k].y * inv);
    }
    for (int k = 0; k < n; ++k) w_out[(size_t)t * n + k] = make_float2((float)y[k].x, (float)y[k].y);
  }
  __syncthreads();
  if (t == 0) info[2] = (uint32_t)sFlags;
}

}  // namespace fmcw
