// fmcw_merge.hip -- the beam merge of include/fmcw.h (fmcw_merge_*): the record list of a multi-beam
// scan in (frame m = scan * n_beams + beam), one fmcw_mplot per local maximum over (beam, range,
// Doppler) out, with the magnitude-weighted offsets that place the target between the beams.
//
// The reference has one receive channel and no beams; with the beamformer in the chain every stage
// after it sees n_frames * n_beams unrelated maps, so a target between two beams is one plot and one
// track per beam.  This is the azimuth centroiding of a surveillance plot extractor, kept in the shape
// of the plotter (fmcw_plots.hip): a list in, a list out, device-resident, stream-ordered, no state.
//
// Four launches (merge_kernel.hpp): k_frame_index, k_merge_find, k_merge_scan, k_merge_emit.  No
// workgroup waits on another, no atomic and no counter that outlives a call.
#include <hip/hip_runtime.h>

#include "internal.hpp"
#include "merge_kernel.hpp"

using fmcw::fail;

static_assert(sizeof(fmcw_mplot) == 32 && sizeof(fmcw_merge_config) == 40, "fmcw.h merge layouts");

namespace {

using namespace fmcw_merge;

int validate(const fmcw_merge_config& c) {
  if (c.n_range < 1 || c.n_range > 65536) return fail(FMCW_EINVAL, "n_range %u (1..65536)", c.n_range);
  if (c.win_beam > 4) return fail(FMCW_EINVAL, "win_beam %u (0..4)", c.win_beam);
  if (c.win_range > 4) return fail(FMCW_EINVAL, "win_range %u (0..4)", c.win_range);
  if (c.win_doppler > 4) return fail(FMCW_EINVAL, "win_doppler %u (0..4)", c.win_doppler);
  if (c.n_doppler < 2 * c.win_doppler + 1 || c.n_doppler > 65536)
    return fail(FMCW_EINVAL, "n_doppler %u (2 win_doppler + 1 = %u .. 65536)", c.n_doppler, 2 * c.win_doppler + 1);
  if (c.n_beams < 1 || c.n_beams > 64) return fail(FMCW_EINVAL, "n_beams %u (1..64)", c.n_beams);
  if (c.beam_wrap > 1) return fail(FMCW_EINVAL, "beam_wrap %u (0 or 1)", c.beam_wrap);
  if (c.beam_wrap && c.n_beams < 2 * c.win_beam + 1)
    return fail(FMCW_EINVAL, "beam_wrap 1 needs n_beams %u >= 2 win_beam + 1 = %u", c.n_beams, 2 * c.win_beam + 1);
  if (c.max_recs < 1 || c.max_recs > 0x7fffffffu) return fail(FMCW_EINVAL, "max_recs %u (1..2^31-1)", c.max_recs);
  if (c.max_maps < c.n_beams || c.max_maps % c.n_beams || c.max_maps > 0x7fffffffu)
    return fail(FMCW_EINVAL, "max_maps %u (a multiple of n_beams %u, below 2^31)", c.max_maps, c.n_beams);
  if (int rc = fmcw::check_device_id(c.device_id)) return rc;
  return FMCW_OK;
}

}  // namespace

struct fmcw_merger {
  fmcw_merge_config cfg;
  uint32_t grid = kMaxGrid;      // workgroups of index / find / emit at most (fmcw_merge_set_grid_for_test)
  uint64_t* masks = nullptr;     // kGroups per tile: 1 bit per record
  uint32_t* tile_cnt = nullptr;  // per tile: peak count, then its exclusive scan
  uint32_t* start = nullptr;     // max_maps + 1 words: the map index
};

extern "C" {

void fmcw_merge_config_default(fmcw_merge_config* cfg) {
  if (!cfg) return;
  cfg->n_range = 1024;
  cfg->n_doppler = 128;
  cfg->n_beams = 1;
  cfg->win_beam = 1;
  cfg->win_range = 1;
  cfg->win_doppler = 1;
  cfg->beam_wrap = 0;
  cfg->max_recs = 1u << 20;
  cfg->max_maps = 1024;
  cfg->device_id = 0;
}

int fmcw_merge_create(const fmcw_merge_config* cfg, fmcw_merger** out) {
  if (!cfg || !out) return fail(FMCW_EINVAL, "null argument");
  *out = nullptr;
  int rc = validate(*cfg);
  if (rc) return rc;
  if ((rc = fmcw::open_device(cfg->device_id))) return rc;
  fmcw_merger* m = new fmcw_merger();
  m->cfg = *cfg;
  const size_t max_tiles = fmcw::tiles_of(cfg->max_recs, MergeTiles::kTile);
  const size_t mask_bytes = max_tiles * MergeTiles::kGroups * sizeof(uint64_t), cnt_bytes = max_tiles * 4;
  const size_t start_bytes = ((size_t)cfg->max_maps + 1) * 4;
  if (!fmcw::alloc_scratch({fmcw::scratch(m->masks, mask_bytes), fmcw::scratch(m->tile_cnt, cnt_bytes),
                            fmcw::scratch(m->start, start_bytes)})) {
    fmcw_merge_destroy(m);
    return fail(FMCW_ENOMEM, "hipMalloc(%zu + %zu + %zu) for the merger's masks, tile counts and map index failed",
                mask_bytes, cnt_bytes, start_bytes);
  }
  *out = m;
  return FMCW_OK;
}

int fmcw_merge_destroy(fmcw_merger* m) {
  if (!m) return FMCW_OK;
  fmcw::free_scratch(m->cfg.device_id, {m->masks, m->tile_cnt, m->start});
  delete m;
  return FMCW_OK;
}

int fmcw_merge_set_grid_for_test(fmcw_merger* m, uint32_t grid) {
  if (!m) return fail(FMCW_EINVAL, "null merger");
  m->grid = fmcw::clamp_grid(grid, kMaxGrid);
  return FMCW_OK;
}

int fmcw_merge_enqueue(fmcw_merger* m, const void* recs_dev, size_t rec_stride, size_t rec_cap,
                       const uint32_t* n_recs_dev, size_t n_maps, fmcw_mplot* out_dev, size_t out_cap,
                       uint32_t* status_dev, void* stream) {
  // what does not depend on the merger first, so that it can be checked without one
  if (int rc = fmcw::check_rec_list_args(recs_dev, rec_stride, rec_cap, n_recs_dev, out_dev, out_cap, status_dev)) return rc;
  if (!m) return fail(FMCW_EINVAL, "null merger");
  if (n_maps > m->cfg.max_maps) return fail(FMCW_EINVAL, "n_maps %zu above max_maps %u", n_maps, m->cfg.max_maps);
  if (n_maps % m->cfg.n_beams)
    return fail(FMCW_EINVAL, "n_maps %zu is not a multiple of n_beams %u", n_maps, m->cfg.n_beams);
  if (hipSetDevice(m->cfg.device_id) != hipSuccess) return fail(FMCW_EHIP, "hipSetDevice");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const fmcw::ListPlan lp = fmcw::plan_list(rec_cap, m->cfg.max_recs, 1, MergeTiles::kTile, m->grid);
  const uint32_t ocap = (uint32_t)std::min<size_t>(out_cap, 0x7fffffffu);      // n < 2^31 merged plots at most
  const RecList l = {static_cast<const uint8_t*>(recs_dev), (uint32_t)rec_stride, lp.cap, n_recs_dev, m->start,
                     (uint32_t)n_maps};
  const WalkGeom g = {m->cfg.n_range, m->cfg.n_doppler, m->cfg.n_beams, m->cfg.win_beam,
                      m->cfg.win_range, m->cfg.win_doppler, m->cfg.beam_wrap};
  const dim3 grid(lp.grid), threads(MergeTiles::kThreads);
  if (lp.tiles) {
    hipLaunchKernelGGL((k_frame_index<MergeTiles::kThreads, MergeTiles::kPer, true>), dim3(lp.index_grid), threads, 0, s,
                       l.recs, l.stride, l.cap, l.n_recs, l.n_groups, m->start);
    if (int rc = fmcw::check_launch("k_frame_index")) return rc;
    hipLaunchKernelGGL(k_merge_find, grid, threads, 0, s, l, g, m->masks, m->tile_cnt);
    if (int rc = fmcw::check_launch("k_merge_find")) return rc;
  }
  hipLaunchKernelGGL(k_merge_scan, dim3(1), dim3(kScanThreads), 0, s, l, m->tile_cnt, status_dev);
  if (int rc = fmcw::check_launch("k_merge_scan")) return rc;
  if (lp.tiles && ocap) {
    hipLaunchKernelGGL(k_merge_emit, grid, threads, 0, s, l, g, m->masks, m->tile_cnt, out_dev, ocap);
    if (int rc = fmcw::check_launch("k_merge_emit")) return rc;
  }
  return FMCW_OK;
}

}  // extern "C"
