// detlist.hip -- the deterministic detection list (radar_core.vhd:396-418): k_det_list orders the
// CFAR kernels' per-tile runs into the caller's list, writes the status words and re-arms the
// handle's per-call counters; k_zero_words arms them where no k_det_list did.
#include <algorithm>

#include "det_sink.hpp"
#include "handle.hpp"

namespace fmcw {
// --------------------------------------------------------------------------------------
// Detection ordering: one pass over the per-tile counts (in tile = (frame, range) order) that
// scans them and copies each tile's run to its final place.
// --------------------------------------------------------------------------------------
// Zeroing of up to three word arrays in one launch (two hipMemsetAsync fills cost ~12 us): the
// caller's status words of a call without a CFAR, and the handle's per-call counters when the
// previous call did not re-arm them (k_det_list).
__global__ void k_zero_words(uint32_t* __restrict__ a, int na, uint32_t* __restrict__ b, int nb,
                             uint32_t* __restrict__ c, int nc) {
  for (int i = threadIdx.x; i < max(na, max(nb, nc)); i += blockDim.x) {
    if (a && i < na) a[i] = 0u;
    if (b && i < nb) b[i] = 0u;
    if (c && i < nc) c[i] = 0u;
  }
}

// Look-back status word of workgroup w: high half = this call's epoch << 2 | error << 1 |
// inclusive, low half = w's detection count (aggregate) or, once inclusive, the count of tiles
// 0 .. kDetTiles (w + 1) - 1.  One 64-bit store / load at agent scope: coherent across the XCDs' L2s.
// The epoch lives in device memory (ep[0], 1 .. 2^30 - 1; ep[1] counts the workgroups that have
// published their inclusive word): every workgroup reads it once at its start, and the last one
// to publish -- when every workgroup of the launch has read it -- advances it and re-arms ep[1].
// So a launch captured into a hipGraph tags its words afresh on every replay (a host-chosen epoch
// would be baked into the graph, and a replay could take a previous replay's word for its own).
constexpr uint32_t kLbIncl = 1u, kLbErr = 2u;
// tiles (= threads) per k_det_list workgroup (256-tile workgroups: 10.7-10.9 / 6.0 / 8.9-9.1 us per
// step at configs 2 / 3 / 5 against 7.4-7.6 / 5.2-5.3 / 7.2-7.3, profiles/r04/detlist/)
constexpr int kDetTiles = 1024;
constexpr uint32_t kLbMaxPolls = 1u << 20;  // >> any real wait (one poll ~1 us): a safety net only

__device__ __forceinline__ void lb_publish(uint64_t* st, uint32_t hi, uint32_t v) {
  __hip_atomic_store(st, ((uint64_t)hi << 32) | v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Round 4: one launch instead of a level-1 scan launch plus a level-2 / copy launch.  Workgroup
// w owns tiles kDetTiles w .. kDetTiles (w + 1) - 1, one per thread: it scans their counts, publishes its aggregate, and takes
// its offset by decoupled look-back -- wave 0 reads the status words of the 64 nearest
// predecessors at once and sums back to the nearest inclusive one.  A workgroup only waits for
// lower ids, which the dispatcher started before it, so the chain drains; the wait is bounded
// all the same, and a workgroup that gives up marks its word (and so every later one) with an
// error the last workgroup reports as every detection lost.  One lane per tile copies the
// tile's records; a tile with more than 8 (a target's row) is copied by the whole wave, 64
// records per step, so one hot tile does not serialise the kernel.  The last workgroup writes
// the status words -- [0] every detection found, [1] of which not stored, [2] / [3] the
// saturation counts the call's K1 / K2 accumulated in the handle's `sat` -- and re-arms the
// handle's per-call counters (overflow use, drops, saturations, the 2-D CFAR launches'
// candidate counters) for the next call: every kernel that uses them ran before this one.
__global__ void __launch_bounds__(kDetTiles)
k_det_list(const fmcw_det* __restrict__ scratch, uint32_t scratch_cap, const uint32_t* __restrict__ wg_base,
           const uint32_t* __restrict__ wg_count, int n, fmcw_det* __restrict__ out, uint32_t cap,
           uint64_t* __restrict__ lb, uint32_t* __restrict__ ep, uint32_t* __restrict__ n_dets,
           uint32_t* __restrict__ counter, uint32_t* __restrict__ sat, uint32_t* __restrict__ k3_ctr, int n_k3) {
  __shared__ int s_wave[kDetTiles / 64 + 1];
  __shared__ uint32_t s_pre, s_err;
  const int lane = threadIdx.x & 63;
  const int w = blockIdx.x;
  const int i = w * kDetTiles + threadIdx.x;
  const uint32_t c = i < n ? wg_count[i] : 0u;
  int agg;
  const uint32_t e = (uint32_t)block_excl_scan<kDetTiles>((int)c, s_wave, agg);
  if (threadIdx.x < 64) {
    // this launch's epoch (set by the previous launch's last publisher: visible at launch start)
    const uint32_t epoch = __builtin_amdgcn_readfirstlane(
        __hip_atomic_load(ep, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    const uint32_t tag = epoch << 2;
    uint32_t pre = 0, err = 0;
    if (w > 0) {
      if (lane == 0) lb_publish(lb + w, tag, (uint32_t)agg);
      int top = w - 1;  // nearest predecessor not yet summed
      uint32_t polls = 0;
      for (;;) {
        const int k = top - lane;
        uint32_t hi = tag | kLbIncl, v = 0;  // below workgroup 0: an inclusive zero
        if (k >= 0) {
          const uint64_t x = __hip_atomic_load(lb + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          hi = (uint32_t)(x >> 32);
          v = (uint32_t)x;
        }
        const bool ready = (hi >> 2) == epoch;
        const uint64_t rdy = __ballot(ready), inc = __ballot(ready && (hi & kLbIncl));
        const int f = inc ? __builtin_ctzll(inc) : 63;            // nearest inclusive lane
        const uint64_t need = f == 63 ? ~0ull : (2ull << f) - 1;  // lanes 0 .. f
        if ((rdy & need) == need) {
          uint32_t t = lane <= f ? v : 0u, te = lane <= f ? (hi & kLbErr) : 0u;
#pragma unroll
          for (int x = 32; x >= 1; x >>= 1) {
            t += (uint32_t)__shfl_xor((int)t, x, 64);
            te |= (uint32_t)__shfl_xor((int)te, x, 64);
          }
          pre += t;
          err |= te;
          if (inc) break;
          top -= 64;
          polls = 0;
        } else if (++polls > kLbMaxPolls) {
          err = kLbErr;
          break;
        }
      }
    }
    if (lane == 0) {
      lb_publish(lb + w, tag | kLbIncl | err, pre + (uint32_t)agg);
      s_pre = pre;
      s_err = err;
      // the last workgroup to get here: every other one has read `epoch` (it did so before
      // publishing), so the next launch's epoch can be set, and the count re-armed
      if (__hip_atomic_fetch_add(ep + 1, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1) {
        const uint32_t nx = (epoch + 1u) & 0x3fffffffu;
        __hip_atomic_store(ep + 1, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(ep, nx ? nx : 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  }
  __syncthreads();
  const uint32_t P = s_pre;
  if (w == (int)gridDim.x - 1) {
    if (threadIdx.x == 0) {
      n_dets[0] = P + (uint32_t)agg;
      n_dets[1] = s_err ? 0xffffffffu : counter[1];
      n_dets[2] = sat ? sat[0] : 0u;
      n_dets[3] = sat ? sat[1] : 0u;
      counter[0] = 0u;
      counter[1] = 0u;
      if (sat) sat[0] = sat[1] = 0u;
    }
    for (int k = threadIdx.x; k < n_k3; k += kDetTiles) k3_ctr[k] = 0u;
  }
  if (!out) return;
  const uint32_t b = c ? wg_base[i] : 0u, o = P + e;
  if (c <= 8)
    for (uint32_t k = 0; k < c; ++k)
      if (b + k < scratch_cap && o + k < cap) out[o + k] = scratch[b + k];
  uint64_t big = __ballot(c > 8);
  while (big) {
    const int l = __builtin_ctzll(big);
    big &= big - 1;
    const uint32_t cl = (uint32_t)__shfl((int)c, l, 64), bl = (uint32_t)__shfl((int)b, l, 64);
    const uint32_t ol = (uint32_t)__shfl((int)o, l, 64);
    for (uint32_t k = lane; k < cl; k += 64)
      if (bl + k < scratch_cap && ol + k < cap) out[ol + k] = scratch[bl + k];
  }
}

size_t det_lb_words(size_t n_tiles) { return (n_tiles + kDetTiles - 1) / kDetTiles; }

int zero_words(uint32_t* w, int n, hipStream_t s) {
  hipLaunchKernelGGL(k_zero_words, dim3(1), dim3(256), 0, s, nullptr, 0, w, n, nullptr, 0);
  return check_launch("k_zero_words");
}

// A call captured into a graph always zeroes the counters (a replay may follow any call, including
// one that stopped early) and leaves the flag as it was: capturing runs nothing, so the device
// state is still the one the flag describes.  Otherwise the flag drops until this call's
// k_det_list is enqueued.
int arm_counters(fmcw_handle* h, hipStream_t s, bool cap) {
  if (!h->counters_armed || cap) {
    hipLaunchKernelGGL(k_zero_words, dim3(1), dim3(256), 0, s, h->counter, 2, h->sat, 2, h->k3_ctr,
                       2 * h->plan.k3_launches);
    if (int rc = check_launch("k_zero_words")) return rc;
  }
  if (!cap) h->counters_armed = false;
  return FMCW_OK;
}

int launch_det_finish(fmcw_handle* h, size_t n_frames, fmcw_det* dets, size_t det_cap,
                      uint32_t* n_dets_dev, uint32_t* sat, hipStream_t s) {
  const Plan& p = h->plan;
  const int n = (int)(n_frames * p.tiles_frame);
  if (n < 1 || (size_t)n > p.n_wg_max) return fail(FMCW_EINVAL, "detection list over %d tiles", n);
  ProfScope ps(&h->prof, FMCW_K_COMPACT);
  // entries past the handle's scratch capacity are never stored: clip to it as well
  const bool copy = dets && det_cap;
  const uint32_t cap = copy ? (uint32_t)std::min<size_t>(det_cap, p.det_scratch_cap) : 0u;
  launch_k(ps, true, k_det_list, dim3((unsigned)det_lb_words(n)), dim3(kDetTiles), 0u, s, (const fmcw_det*)h->det_scratch,
           p.det_scratch_cap, (const uint32_t*)h->wg_base, (const uint32_t*)h->wg_count, n,
           copy ? dets : (fmcw_det*)nullptr, cap, h->lb_status, h->det_epoch, n_dets_dev, h->counter, sat, h->k3_ctr,
           2 * p.k3_launches);
  return check_launch("k_det_list");
}

}  // namespace fmcw
