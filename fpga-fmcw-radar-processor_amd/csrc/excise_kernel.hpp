// excise_kernel.hpp -- k_excise: the interference exciser of include/fmcw.h "Interference excision":
// per chirp, the power's exact order statistic, the flags against alpha x that level, their dilation
// and the repair of every run, in one pass over the ADC cube.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/fmcw.h"

// Every step of the specification is one individually rounded fp32 operation: no multiply and add of
// this file may be contracted into an FMA.
#pragma clang fp contract(off)

namespace fmcw {

// --------------------------------------------------------------------------------------
// Geometry.  A line is one chirp: ns complex samples, contiguous in the cube.  Persistent workgroups of
// 256 threads stride over the lines, one line at a time.  A line is read once, with 16-byte loads:
// vector vi = j * 256 + tid (j < NV) holds the V samples vi * V .. vi * V + V - 1 (V = 2 complex64 or 4
// f16 / int16 pairs), and stays in registers as loaded, so that a sample outside every run is stored
// with the bits it came with.  Lines shorter than 256 vectors leave the upper threads without one.
//
// Per line:
//   (a) load, p = fl(fl(re re) + fl(im im)); the powers stay in registers as bit patterns (p >= +0, so
//       their order as unsigned integers is their order as numbers) and go to LDS once;
//   (b) the k-th smallest pattern by bisection from bit 30 down: a candidate bit stays when at most k
//       powers lie below the candidate.  A wave's count is the popcount of its compares' lane masks,
//       the four waves' counts meet in LDS (two slots, by the parity of the bit: one barrier per bit);
//   (c) flags in sample order: thread tid reads p[i * 256 + tid] from LDS, and the compare's 64-bit
//       lane mask is two mask words of the line;
//   (d) dilation, one thread per mask word: the OR of the word's neighbourhood shifted by 1 .. guard
//       (guard <= 32: the two adjacent words suffice); the words' popcounts add up in LDS;
//   (e) a clean line is copied (out of place) or left alone (in place).  Otherwise every thread
//       repairs the samples of its own vectors whose bit is set -- for INTERP the run's ends come
//       from bit scans over the dilated words, the two neighbours from the input cube, which no
//       repair writes -- and stores its vectors (in place: those it changed).
// Thread 0 sums the status words over the workgroup's lines and adds them once, with integer atomics.
// --------------------------------------------------------------------------------------
constexpr int kExNT = 256;   // threads per workgroup

struct ExciseArgs {
  uint32_t ns;        // samples per line
  uint32_t n_lines;   // n_frames x n_rx x n_doppler
  uint32_t k;         // 0-based ascending rank of the level
  uint32_t guard;
  int mode;           // fmcw_excise_mode
  float alpha;
  int in_place;       // out == cube
};

// The cube's element types: V samples per 16-byte vector; sample v of a vector as fp32 (exact) and
// back (f16: nearest even; int16: half to even, a convex combination of two int16 values).
struct ExF32 {
  static constexpr int V = 2;
  __device__ __forceinline__ static float2 get(const uint32_t (&w)[4], int v) {
    return make_float2(__uint_as_float(w[2 * v]), __uint_as_float(w[2 * v + 1]));
  }
  __device__ __forceinline__ static void set(uint32_t (&w)[4], int v, float2 x) {
    w[2 * v] = __float_as_uint(x.x);
    w[2 * v + 1] = __float_as_uint(x.y);
  }
  __device__ __forceinline__ static float2 load1(const void* cube, size_t idx) {
    return reinterpret_cast<const float2*>(cube)[idx];
  }
};
struct ExF16 {
  static constexpr int V = 4;
  typedef _Float16 h2 __attribute__((ext_vector_type(2)));
  __device__ __forceinline__ static float2 word(uint32_t u) {
    const h2 h = __builtin_bit_cast(h2, u);
    return make_float2((float)h[0], (float)h[1]);
  }
  __device__ __forceinline__ static float2 get(const uint32_t (&w)[4], int v) { return word(w[v]); }
  __device__ __forceinline__ static void set(uint32_t (&w)[4], int v, float2 x) {
    h2 h;
    h[0] = (_Float16)x.x;
    h[1] = (_Float16)x.y;
    w[v] = __builtin_bit_cast(uint32_t, h);
  }
  __device__ __forceinline__ static float2 load1(const void* cube, size_t idx) {
    return word(reinterpret_cast<const uint32_t*>(cube)[idx]);
  }
};
struct ExI16 {
  static constexpr int V = 4;
  __device__ __forceinline__ static float2 word(uint32_t u) {
    return make_float2((float)(int16_t)(u & 0xffffu), (float)(int16_t)(u >> 16));
  }
  __device__ __forceinline__ static float2 get(const uint32_t (&w)[4], int v) { return word(w[v]); }
  __device__ __forceinline__ static void set(uint32_t (&w)[4], int v, float2 x) {
    const uint32_t re = (uint32_t)__float2int_rn(x.x) & 0xffffu, im = (uint32_t)__float2int_rn(x.y) & 0xffffu;
    w[v] = re | (im << 16);
  }
  __device__ __forceinline__ static float2 load1(const void* cube, size_t idx) {
    return word(reinterpret_cast<const uint32_t*>(cube)[idx]);
  }
};

// The dilated word of b between its neighbours a (samples below) and c (above): the OR of the three
// words' bits within `guard` of each bit of b.
__host__ __device__ inline uint32_t excise_dilate(uint32_t a, uint32_t b, uint32_t c, uint32_t guard) {
  const uint64_t below = ((uint64_t)b << 32) | a, above = ((uint64_t)c << 32) | b;
  uint32_t g = b;
  for (uint32_t s = 1; s <= guard; ++s) g |= (uint32_t)((below << s) >> 32) | (uint32_t)(above >> s);
  return g;
}

// First and last sample of the run of set bits around sample n (whose bit is set) in the nw words g.
__host__ __device__ inline int excise_run_start(const uint32_t* g, int n) {
  int w = n >> 5;
  uint32_t clear = ~g[w] & ((1u << (n & 31)) - 1u);   // the clear bits below n in its own word
  while (clear == 0) {
    if (--w < 0) return 0;
    clear = ~g[w];
  }
  return (w << 5) + 32 - __builtin_clz(clear);
}
__host__ __device__ inline int excise_run_end(const uint32_t* g, int n, int nw) {
  int w = n >> 5;
  uint32_t clear = ~g[w] & ~((2u << (n & 31)) - 1u);   // the clear bits above n in its own word
  while (clear == 0) {
    if (++w >= nw) return (nw << 5) - 1;
    clear = ~g[w];
  }
  return (w << 5) + __builtin_ctz(clear) - 1;
}

// The linear interpolation of sample n of the run [a, b] between lo = x[a - 1] and hi = x[b + 1]:
// three rounded operations per component after one correctly rounded division.
__host__ __device__ inline float excise_lerp(float lo, float hi, float t) {
  const float d = hi - lo;
  const float td = t * d;
  return lo + td;
}

// The repaired value of sample n (INTERP), out of line: repairs are rare, and a kernel holds up to 32
// of them unrolled.
template <class L>
__device__ __noinline__ float2 excise_interp(const uint32_t* g, const void* cube, size_t line0, int n, int ns) {
  const int a = excise_run_start(g, n), b = excise_run_end(g, n, ns >> 5);
  const bool has_lo = a > 0, has_hi = b < ns - 1;
  if (!has_lo && !has_hi) return make_float2(0.f, 0.f);
  const float2 lo = L::load1(cube, line0 + (size_t)(has_lo ? a - 1 : b + 1));
  if (!has_hi) return lo;
  const float2 hi = L::load1(cube, line0 + (size_t)(b + 1));
  if (!has_lo) return hi;
  const float t = __fdiv_rn((float)(n - a + 1), (float)(b - a + 2));
  return make_float2(excise_lerp(lo.x, hi.x, t), excise_lerp(lo.y, hi.y, t));
}

// L: the cube's element type; NV: 16-byte vectors per thread, max(1, ns / V / 256).
template <class L, int NV>
__global__ void __launch_bounds__(kExNT)
k_excise(const uint4* cube, uint4* out, ExciseArgs g, uint32_t* __restrict__ mask, uint32_t* __restrict__ counts,
         uint32_t* __restrict__ status) {
  constexpr int V = L::V;
  constexpr int kSamples = NV * V * kExNT;   // >= ns, >= 256
  __shared__ __attribute__((aligned(16))) uint32_t s_p[kSamples];   // the powers' bit patterns
  __shared__ uint32_t s_f[kSamples / 32], s_g[kSamples / 32];       // flags; dilated flags
  __shared__ uint32_t s_cnt[2][kExNT / 64];
  __shared__ uint32_t s_tot[2];                                     // samples repaired, flagged
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ns = (int)g.ns, nw = ns >> 5;
  const uint32_t nvec = g.ns / V;
  const float alpha = g.alpha;
  uint32_t st_rep = 0, st_lines = 0, st_flag = 0, st_heavy = 0;   // thread 0's

  for (uint32_t line = blockIdx.x; line < g.n_lines; line += gridDim.x) {
    const size_t vec0 = (size_t)line * nvec;
    uint32_t raw[NV][4], pb[NV][V];
    // (a)
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const uint32_t vi = (uint32_t)(j * kExNT + tid);
      if (vi < nvec) {
        const uint4 t = cube[vec0 + vi];
        raw[j][0] = t.x, raw[j][1] = t.y, raw[j][2] = t.z, raw[j][3] = t.w;
#pragma unroll
        for (int v = 0; v < V; ++v) {
          const float2 x = L::get(raw[j], v);
          const float rr = x.x * x.x, ii = x.y * x.y;
          pb[j][v] = __float_as_uint(rr + ii);
          s_p[vi * V + v] = pb[j][v];
        }
      } else {
#pragma unroll
        for (int v = 0; v < V; ++v) pb[j][v] = 0xffffffffu;   // below no candidate
      }
    }
    // (b)
    uint32_t level = 0;
    for (int bit = 30; bit >= 0; --bit) {
      const uint32_t cand = level | (1u << bit);
      uint32_t below = 0;
#pragma unroll
      for (int j = 0; j < NV; ++j)
#pragma unroll
        for (int v = 0; v < V; ++v) below += (uint32_t)__popcll(__ballot(pb[j][v] < cand));
      if (lane == 0) s_cnt[bit & 1][wave] = below;
      __syncthreads();
      const uint32_t* const c = s_cnt[bit & 1];
      if (c[0] + c[1] + c[2] + c[3] <= g.k) level = cand;
    }
    const float thr = alpha * __uint_as_float(level);
    // (c)
    for (int n0 = 0; n0 < kSamples && n0 < max(ns, kExNT); n0 += kExNT) {
      const int n = n0 + tid;
      const bool f = n < ns && __uint_as_float(s_p[n]) > thr;
      const unsigned long long m = __ballot(f);
      if (lane == 0) {
        s_f[(n0 >> 5) + 2 * wave] = (uint32_t)m;
        s_f[(n0 >> 5) + 2 * wave + 1] = (uint32_t)(m >> 32);
      }
    }
    if (tid == 0) s_tot[0] = s_tot[1] = 0;
    __syncthreads();
    // (d)
    if (tid < nw) {
      const uint32_t b = s_f[tid];
      const uint32_t gw = excise_dilate(tid > 0 ? s_f[tid - 1] : 0u, b, tid + 1 < nw ? s_f[tid + 1] : 0u, g.guard);
      s_g[tid] = gw;
      if (mask) mask[(size_t)line * nw + tid] = gw;
      if (gw) atomicAdd(&s_tot[0], (uint32_t)__popc(gw));
      if (b) atomicAdd(&s_tot[1], (uint32_t)__popc(b));
    }
    __syncthreads();
    const uint32_t n_rep = s_tot[0];
    if (tid == 0) {
      if (counts) counts[line] = n_rep;
      st_rep += n_rep;
      st_lines += n_rep ? 1u : 0u;
      st_flag += s_tot[1];
      st_heavy += n_rep > g.ns / 2 ? 1u : 0u;
    }
    // (e)
    if (n_rep == 0 && g.in_place) continue;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const uint32_t vi = (uint32_t)(j * kExNT + tid);
      if (vi >= nvec) continue;
      uint32_t bits = 0;
      if (n_rep) {
        const uint32_t n0 = vi * V;
        bits = (s_g[n0 >> 5] >> (n0 & 31)) & ((1u << V) - 1u);
#pragma unroll
        for (int v = 0; v < V; ++v)
          if (bits >> v & 1u) {
            float2 x = make_float2(0.f, 0.f);
            if (g.mode == FMCW_EXCISE_INTERP && n_rep < g.ns)
              x = excise_interp<L>(s_g, cube, (size_t)line * g.ns, (int)n0 + v, ns);
            L::set(raw[j], v, x);
          }
      }
      if (bits || !g.in_place) out[vec0 + vi] = make_uint4(raw[j][0], raw[j][1], raw[j][2], raw[j][3]);
    }
  }
  if (tid == 0) {
    if (st_rep) atomicAdd(&status[0], st_rep);
    if (st_lines) atomicAdd(&status[1], st_lines);
    if (st_flag) atomicAdd(&status[2], st_flag);
    if (st_heavy) atomicAdd(&status[3], st_heavy);
  }
}

}  // namespace fmcw
