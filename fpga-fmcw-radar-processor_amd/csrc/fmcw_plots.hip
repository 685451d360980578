// fmcw_plots.hip -- plot extraction ("peak grouping") of include/fmcw.h: the ordered detection
// list of fmcw_enqueue / fmcw_cfar in, one fmcw_plot per local-maximum detection out.
//
// The reference has no such stage: radar_core streams every non-zero CFAR output straight into
// tws_tracker (radar_core.vhd:413-438), which keeps a scan's first MAX_DETS = 64 of them
// (tws_tracker.vhd COLLECT).  A point target's Hamming main lobe and Doppler sidelobes are dozens
// of detections, so the tracker's slots fill with the nearest target's cells; this stage reduces
// each cluster to one report before the tracker.
//
// The only input is the sorted record list (it carries the magnitudes): no map, no per-cell mask.
// A workgroup owns a tile of kTile consecutive records and stages them, with kHalo records on
// either side, in LDS as (64-bit key, magnitude).  A lane owns a detection P = (f, r, d); for each
// row r + dr of its window it takes a lower-bound search for the key (f, r + dr, first column) --
// bounded to the (|dr| + 1) n_doppler records either side of P, where the row must lie because the
// list holds a cell at most once -- and reads the at most 2 win_doppler + 1 entries that follow.
// The Doppler wrap splits a row into at most two column runs.  Probes inside the staged span read
// LDS, the others global memory.
//
// Three launches, no workgroup waits on another, no atomic and no counter that outlives a call:
//   k_plots_find   peak test per detection (stops at the first larger neighbour): one 64-bit
//                  ballot mask per 64 records, one peak count per tile
//   k_plots_scan   one workgroup: exclusive scan of the tile counts (det_sink.hpp tile_offsets_scan,
//                  the detectors' scan), and the two status words
//   k_plots_emit   the peaks' rank from the tile offset and the masks; each peak below plot_cap
//                  walks its window once more for the sums and writes its plot
// Every word the later launches read is written by the earlier ones in the same call (tile counts
// and masks of all tiles below n), so there is nothing to zero between calls and a captured graph
// replays as it is.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "det_sink.hpp"
#include "internal.hpp"
#include "plots_window.hpp"

using fmcw::fail;

static_assert(sizeof(fmcw_plot) == 32 && sizeof(fmcw_plots_config) == 24, "fmcw.h plot layouts");

namespace {

using namespace fmcw_plots;

constexpr int kThreads = 256;                // 4 waves
constexpr int kPer = 4;                      // records per lane and tile
constexpr uint32_t kTile = kThreads * kPer;  // records per tile
constexpr uint32_t kHalo = 512;              // staged either side of the tile
constexpr uint32_t kStage = kTile + 2 * kHalo;
constexpr int kGroups = kTile / 64;          // ballot masks per tile
constexpr uint32_t kMaxGrid = 4096;          // workgroups of find / emit (they stride over the tiles)
constexpr int kScanThreads = 1024;

__device__ __forceinline__ uint32_t examined(const uint32_t* n_dets, uint32_t cap) { return min(n_dets[0], cap); }

// Stage tile t's span; every lane of the workgroup calls it.  The caller syncs after it.
__device__ __forceinline__ ListView stage_tile(const fmcw_det* __restrict__ dets, uint32_t n, uint32_t base,
                                               uint64_t* s_key, float* s_mag) {
  ListView v;
  v.dets = dets;
  v.n = n;
  v.s_lo = base > kHalo ? base - kHalo : 0u;
  v.s_n = min(n, base + kTile + kHalo) - v.s_lo;  // <= kStage (base < n)
  v.s_key = s_key;
  v.s_mag = s_mag;
  for (uint32_t j = threadIdx.x; j < v.s_n; j += kThreads) {
    const fmcw_det r = dets[v.s_lo + j];
    s_key[j] = make_key(r.frame, r.range, r.doppler);
    s_mag[j] = r.mag;
  }
  return v;
}

__global__ void __launch_bounds__(kThreads) k_plots_find(const fmcw_det* __restrict__ dets, uint32_t cap,
                                                          const uint32_t* __restrict__ n_dets, PlotGeom g,
                                                          uint64_t* __restrict__ masks, uint32_t* __restrict__ tile_cnt) {
  __shared__ uint64_t s_key[kStage];
  __shared__ float s_mag[kStage];
  __shared__ uint32_t s_cnt[kGroups];
  const uint32_t n = examined(n_dets, cap);
  const uint32_t n_tiles = (n + kTile - 1) / kTile;
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (uint32_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const uint32_t base = t * kTile;
    __syncthreads();  // the previous tile's readers are done with the staging arrays
    const ListView v = stage_tile(dets, n, base, s_key, s_mag);
    __syncthreads();
    for (int k = 0; k < kPer; ++k) {
      const uint32_t i = base + k * kThreads + tid;
      bool peak = false;
      if (i < n) {
        const uint64_t kp = v.key(i);
        const float mp = v.mag(i);
        peak = true;
        visit_window(v, g, i, (uint32_t)(kp >> 32), (uint32_t)(kp >> 16) & 0xffffu, (uint32_t)kp & 0xffffu,
                     [&](uint32_t q, float m, int, int) {
                       if (q != i && (m > mp || (m == mp && q < i))) peak = false;
                       return peak;
                     });
      }
      const uint64_t m = __ballot(peak);
      if (lane == 0) {
        masks[(size_t)t * kGroups + k * (kThreads / 64) + wave] = m;
        s_cnt[k * (kThreads / 64) + wave] = (uint32_t)__popcll(m);
      }
    }
    __syncthreads();
    if (tid == 0) {
      uint32_t c = 0;
      for (int j = 0; j < kGroups; ++j) c += s_cnt[j];
      tile_cnt[t] = c;
    }
  }
}

// One workgroup: tile_cnt -> exclusive scan in place, and the status words.
__global__ void __launch_bounds__(kScanThreads) k_plots_scan(uint32_t cap, const uint32_t* __restrict__ n_dets,
                                                              uint32_t* __restrict__ tile_cnt,
                                                              uint32_t* __restrict__ n_plots) {
  const uint32_t found = n_dets[0];
  const uint32_t n = min(found, cap);
  const uint32_t n_tiles = (n + kTile - 1) / kTile;   // <= 2^21, a tile has at most kTile peaks
  const uint32_t sum = fmcw::tile_offsets_scan<kScanThreads>(tile_cnt, tile_cnt, (int)n_tiles);
  if (threadIdx.x == 0) {
    n_plots[0] = sum;
    n_plots[1] = found - n;
  }
}

__global__ void __launch_bounds__(kThreads) k_plots_emit(const fmcw_det* __restrict__ dets, uint32_t cap,
                                                          const uint32_t* __restrict__ n_dets, PlotGeom g,
                                                          const uint64_t* __restrict__ masks,
                                                          const uint32_t* __restrict__ tile_off,
                                                          fmcw_plot* __restrict__ plots, uint32_t plot_cap) {
  __shared__ uint64_t s_key[kStage];
  __shared__ float s_mag[kStage];
  __shared__ uint64_t s_m[kGroups];
  const uint32_t n = examined(n_dets, cap);
  const uint32_t n_tiles = (n + kTile - 1) / kTile;
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (uint32_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const uint32_t base = t * kTile;
    const uint32_t off = tile_off[t];
    if (off >= plot_cap) break;  // offsets only grow with t: nothing left to write for this workgroup
    __syncthreads();
    const ListView v = stage_tile(dets, n, base, s_key, s_mag);
    if (tid < kGroups) s_m[tid] = masks[(size_t)t * kGroups + tid];
    __syncthreads();
    for (int k = 0; k < kPer; ++k) {
      const int grp = k * (kThreads / 64) + (int)wave;  // records base + 64 grp ..: list order
      uint32_t rank = off;
      for (int j = 0; j < grp; ++j) rank += (uint32_t)__popcll(s_m[j]);
      const uint64_t m = s_m[grp];
      rank += (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
      const uint32_t i = base + k * kThreads + tid;
      if (!((m >> lane) & 1ull) || rank >= plot_cap) continue;
      const fmcw_det p = dets[i];
      uint32_t cells = 0;
      float s = 0.f, sr = 0.f, sd = 0.f;
      visit_window(v, g, i, p.frame, p.range, p.doppler, [&](uint32_t, float mq, int dr, int dd) {
        ++cells;
        s += mq;
        sr += mq * (float)dr;
        sd += mq * (float)dd;
        return true;
      });
      const bool ok = s != 0.f && fabsf(s) <= 3.402823466e38f;  // finite (NaN compares false)
      fmcw_plot o;
      o.frame = p.frame;
      o.range = p.range;
      o.doppler = p.doppler;
      o.mag = p.mag;
      o.threshold = p.threshold;
      o.n_cells = cells;
      o.sum_mag = s;
      o.d_range = ok ? sr / s : 0.f;
      o.d_doppler = ok ? sd / s : 0.f;
      plots[rank] = o;
    }
  }
}

int validate(const fmcw_plots_config& c) {
  if (c.n_range < 1 || c.n_range > 65536) return fail(FMCW_EINVAL, "n_range %u (1..65536)", c.n_range);
  if (c.win_range > 4) return fail(FMCW_EINVAL, "win_range %u (0..4)", c.win_range);
  if (c.win_doppler > 4) return fail(FMCW_EINVAL, "win_doppler %u (0..4)", c.win_doppler);
  if (c.n_doppler < 2 * c.win_doppler + 1 || c.n_doppler > 65536)
    return fail(FMCW_EINVAL, "n_doppler %u (2 win_doppler + 1 = %u .. 65536)", c.n_doppler, 2 * c.win_doppler + 1);
  if (c.max_dets < 1 || c.max_dets > 0x7fffffffu) return fail(FMCW_EINVAL, "max_dets %u (1..2^31-1)", c.max_dets);
  if (int rc = fmcw::check_device_id(c.device_id)) return rc;
  return FMCW_OK;
}

}  // namespace

struct fmcw_plotter {
  fmcw_plots_config cfg;
  uint32_t max_tiles = 0;
  uint32_t grid = kMaxGrid;      // workgroups of find / emit at most (fmcw_plots_set_grid_for_test)
  uint64_t* masks = nullptr;     // kGroups per tile: 1 bit per record
  uint32_t* tile_cnt = nullptr;  // per tile: peak count, then its exclusive scan
};

extern "C" {

void fmcw_plots_config_default(fmcw_plots_config* cfg) {
  if (!cfg) return;
  cfg->n_range = 1024;
  cfg->n_doppler = 128;
  cfg->win_range = 1;
  cfg->win_doppler = 1;
  cfg->max_dets = 1u << 20;
  cfg->device_id = 0;
}

int fmcw_plots_create(const fmcw_plots_config* cfg, fmcw_plotter** out) {
  if (!cfg || !out) return fail(FMCW_EINVAL, "null argument");
  *out = nullptr;
  int rc = validate(*cfg);
  if (rc) return rc;
  if ((rc = fmcw::open_device(cfg->device_id))) return rc;
  fmcw_plotter* p = new fmcw_plotter();
  p->cfg = *cfg;
  p->max_tiles = (uint32_t)(((uint64_t)cfg->max_dets + kTile - 1) / kTile);
  const size_t mask_bytes = (size_t)p->max_tiles * kGroups * sizeof(uint64_t), cnt_bytes = (size_t)p->max_tiles * 4;
  if (hipMalloc(reinterpret_cast<void**>(&p->masks), mask_bytes) != hipSuccess ||
      hipMalloc(reinterpret_cast<void**>(&p->tile_cnt), cnt_bytes) != hipSuccess) {
    (void)hipGetLastError();
    fmcw_plots_destroy(p);
    return fail(FMCW_ENOMEM, "hipMalloc(%zu + %zu) for the plotter's masks and tile counts failed", mask_bytes,
                 cnt_bytes);
  }
  *out = p;
  return FMCW_OK;
}

int fmcw_plots_destroy(fmcw_plotter* p) {
  if (!p) return FMCW_OK;
  hipSetDevice(p->cfg.device_id);
  if (p->masks) hipFree(p->masks);
  if (p->tile_cnt) hipFree(p->tile_cnt);
  delete p;
  return FMCW_OK;
}

int fmcw_plots_set_grid_for_test(fmcw_plotter* p, uint32_t grid) {
  if (!p) return fail(FMCW_EINVAL, "null plotter");
  p->grid = fmcw::clamp_grid(grid, kMaxGrid);
  return FMCW_OK;
}

int fmcw_plots_enqueue(fmcw_plotter* p, const fmcw_det* dets_dev, size_t det_cap, const uint32_t* n_dets_dev,
                       fmcw_plot* plots_dev, size_t plot_cap, uint32_t* n_plots_dev, void* stream) {
  if (!p || !n_dets_dev || !n_plots_dev) return fail(FMCW_EINVAL, "null argument");
  if (det_cap && !dets_dev) return fail(FMCW_EINVAL, "null dets_dev with det_cap %zu", det_cap);
  if (plot_cap && !plots_dev) return fail(FMCW_EINVAL, "null plots_dev with plot_cap %zu", plot_cap);
  if (hipSetDevice(p->cfg.device_id) != hipSuccess) return fail(FMCW_EHIP, "hipSetDevice");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const uint32_t cap = (uint32_t)std::min<size_t>(det_cap, p->cfg.max_dets);  // n = min(n_dets_dev[0], cap)
  const uint32_t pcap = (uint32_t)std::min<size_t>(plot_cap, 0x7fffffffu);     // n < 2^31 plots at most
  const uint32_t tiles = (uint32_t)(((uint64_t)cap + kTile - 1) / kTile);       // <= max_tiles
  const PlotGeom g = {p->cfg.n_range, p->cfg.n_doppler, p->cfg.win_range, p->cfg.win_doppler};
  const dim3 grid(std::min(tiles, p->grid));
  if (tiles) {
    hipLaunchKernelGGL(k_plots_find, grid, dim3(kThreads), 0, s, dets_dev, cap, n_dets_dev, g, p->masks, p->tile_cnt);
    if (int rc = fmcw::check_launch("k_plots_find")) return rc;
  }
  hipLaunchKernelGGL(k_plots_scan, dim3(1), dim3(kScanThreads), 0, s, cap, n_dets_dev, p->tile_cnt, n_plots_dev);
  if (int rc = fmcw::check_launch("k_plots_scan")) return rc;
  if (tiles && pcap) {
    hipLaunchKernelGGL(k_plots_emit, grid, dim3(kThreads), 0, s, dets_dev, cap, n_dets_dev, g, p->masks, p->tile_cnt,
                       plots_dev, pcap);
    if (int rc = fmcw::check_launch("k_plots_emit")) return rc;
  }
  return FMCW_OK;
}

}  // extern "C"
