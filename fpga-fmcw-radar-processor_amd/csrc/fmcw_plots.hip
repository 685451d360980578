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
// the first bounded to the (win_range + 1) n_doppler records before P, every later one to the
// n_doppler records after the one before it, where the row must lie because the list holds a cell
// at most once -- and reads the at most 2 win_doppler + 1 entries that follow.  The Doppler wrap
// splits a row into at most two column runs.  Probes inside the staged span read LDS, the others
// global memory.  The walk is the beam merger's (rec_window.hpp visit_neighbourhood) with one beam.
//
// Three launches (rec_tiles.hpp), no workgroup waits on another, no atomic and no counter that
// outlives a call:
//   k_plots_find   find_peaks: peak test per detection (stops at the first larger neighbour): one
//                  64-bit ballot mask per 64 records, one peak count per tile
//   k_plots_scan   one workgroup: exclusive scan of the tile counts (det_sink.hpp tile_offsets_scan,
//                  the detectors' scan), and the two status words
//   k_plots_emit   emit_peaks: the peaks' rank from the tile offset and the masks; each peak below
//                  plot_cap walks its window once more for the sums and writes its plot
// Every word the later launches read is written by the earlier ones in the same call (tile counts
// and masks of all tiles below n), so there is nothing to zero between calls and a captured graph
// replays as it is.
#include <hip/hip_runtime.h>

#include "internal.hpp"
#include "rec_tiles.hpp"

using fmcw::fail;

static_assert(sizeof(fmcw_plot) == 32 && sizeof(fmcw_plots_config) == 24, "fmcw.h plot layouts");

namespace {

using namespace fmcw_rec;

using PlotTiles = Tiles<256, 4>;             // 4 waves, 4 records per lane and tile
constexpr uint32_t kHalo = 512;              // staged either side of the tile
constexpr uint32_t kMaxGrid = 4096;          // workgroups of find / emit (they stride over the tiles)
constexpr int kScanThreads = 1024;

__global__ void __launch_bounds__(PlotTiles::kThreads) k_plots_find(RecList l, WalkGeom g, uint64_t* __restrict__ masks,
                                                                     uint32_t* __restrict__ tile_cnt) {
  find_peaks<PlotTiles, kHalo>(l, g, masks, tile_cnt);
}

// One workgroup: tile_cnt -> exclusive scan in place, and the two status words.
__global__ void __launch_bounds__(kScanThreads) k_plots_scan(RecList l, uint32_t* __restrict__ tile_cnt,
                                                              uint32_t* __restrict__ n_plots) {
  scan_status<kScanThreads>(l, tile_cnt, PlotTiles::count(in_use(l)), n_plots);
}

__global__ void __launch_bounds__(PlotTiles::kThreads) k_plots_emit(RecList l, WalkGeom g, const uint64_t* __restrict__ masks,
                                                                     const uint32_t* __restrict__ tile_off,
                                                                     fmcw_plot* __restrict__ plots, uint32_t plot_cap) {
  emit_peaks<PlotTiles, kHalo>(l, g, masks, tile_off, plot_cap, [&](uint32_t rank, const RecView& v, const PeakSums& p) {
    fmcw_plot o;
    o.frame = p.m;
    o.range = (uint16_t)p.r;
    o.doppler = (uint16_t)p.d;
    o.mag = v.mag(p.i);
    o.threshold = __uint_as_float(v.word(p.i)[3]);
    o.n_cells = p.cnt;
    o.sum_mag = p.s;
    o.d_range = p.centre(p.sr);
    o.d_doppler = p.centre(p.sd);
    plots[rank] = o;
  });
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
  const size_t max_tiles = fmcw::tiles_of(cfg->max_dets, PlotTiles::kTile);
  const size_t mask_bytes = max_tiles * PlotTiles::kGroups * sizeof(uint64_t), cnt_bytes = max_tiles * 4;
  if (!fmcw::alloc_scratch({fmcw::scratch(p->masks, mask_bytes), fmcw::scratch(p->tile_cnt, cnt_bytes)})) {
    fmcw_plots_destroy(p);
    return fail(FMCW_ENOMEM, "hipMalloc(%zu + %zu) for the plotter's masks and tile counts failed", mask_bytes,
                 cnt_bytes);
  }
  *out = p;
  return FMCW_OK;
}

int fmcw_plots_destroy(fmcw_plotter* p) {
  if (!p) return FMCW_OK;
  fmcw::free_scratch(p->cfg.device_id, {p->masks, p->tile_cnt});
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
  const fmcw::ListPlan lp = fmcw::plan_list(det_cap, p->cfg.max_dets, 1, PlotTiles::kTile, p->grid);
  const uint32_t pcap = (uint32_t)std::min<size_t>(plot_cap, 0x7fffffffu);     // n < 2^31 plots at most
  const RecList l = {reinterpret_cast<const uint8_t*>(dets_dev), (uint32_t)sizeof(fmcw_det), lp.cap, n_dets_dev, nullptr, 0};
  // one beam per scan: the window is the merger's neighbourhood without the beam axis (rec_window.hpp)
  const WalkGeom g = {p->cfg.n_range, p->cfg.n_doppler, 1, 0, p->cfg.win_range, p->cfg.win_doppler, 0};
  const dim3 grid(lp.grid), threads(PlotTiles::kThreads);
  if (lp.tiles) {
    hipLaunchKernelGGL(k_plots_find, grid, threads, 0, s, l, g, p->masks, p->tile_cnt);
    if (int rc = fmcw::check_launch("k_plots_find")) return rc;
  }
  hipLaunchKernelGGL(k_plots_scan, dim3(1), dim3(kScanThreads), 0, s, l, p->tile_cnt, n_plots_dev);
  if (int rc = fmcw::check_launch("k_plots_scan")) return rc;
  if (lp.tiles && pcap) {
    hipLaunchKernelGGL(k_plots_emit, grid, threads, 0, s, l, g, p->masks, p->tile_cnt, plots_dev, pcap);
    if (int rc = fmcw::check_launch("k_plots_emit")) return rc;
  }
  return FMCW_OK;
}

}  // extern "C"
