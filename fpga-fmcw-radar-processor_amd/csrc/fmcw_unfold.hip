// fmcw_unfold.hip -- the velocity unfolder of include/fmcw.h (fmcw_unfold_*): the record list of a
// PRF-staggered sequence of scans in, one fmcw_vplot per target and dwell out, with the unambiguous
// radial velocity that the K PRFs of the dwell agree on.
//
// The reference's testbench staggers three PRFs so that no target stays at a blind speed, but nothing
// behind its CFAR uses the stagger: a fast target's Doppler bin changes from scan to scan.  This is
// the M-of-K coincidence unfolding of a medium-PRF radar, kept in the shape of the beam merger
// (fmcw_merge.hip): a list in, a list out, device-resident, stream-ordered, no state.
//
// Five launches (unfold_kernel.hpp): k_frame_index and k_unfold_dwells (the frame index and, from it,
// the index of the (dwell, record) pairs), k_unfold_find, k_unfold_scan, k_unfold_emit.  No workgroup
// waits on another, no atomic and no counter that outlives a call.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "internal.hpp"
#include "unfold_kernel.hpp"

using fmcw::fail;

static_assert(sizeof(fmcw_vplot) == 32 && sizeof(fmcw_unfold_config) == 92, "fmcw.h unfold layouts");

namespace {

using namespace fmcw_unfold;
using fmcw_rec::k_frame_index;

uint32_t dwells_per_record(const fmcw_unfold_config& c) { return (c.n_prf + c.step - 1) / c.step; }

int validate(const fmcw_unfold_config& c) {
  if (c.n_range < 1 || c.n_range > 65536) return fail(FMCW_EINVAL, "n_range %u (1..65536)", c.n_range);
  if (c.tol_range > 4) return fail(FMCW_EINVAL, "tol_range %u (0..4)", c.tol_range);
  if (c.tol_doppler > 4) return fail(FMCW_EINVAL, "tol_doppler %u (0..4)", c.tol_doppler);
  if (c.n_doppler < 2 * c.tol_doppler + 1 || c.n_doppler > 65536)
    return fail(FMCW_EINVAL, "n_doppler %u (2 tol_doppler + 1 = %u .. 65536)", c.n_doppler, 2 * c.tol_doppler + 1);
  if (c.n_prf < 2 || c.n_prf > 8) return fail(FMCW_EINVAL, "n_prf %u (2..8)", c.n_prf);
  uint32_t p_min = 4096;
  for (uint32_t k = 0; k < c.n_prf; ++k) {
    if (c.prf_units[k] < 1 || c.prf_units[k] > 4096) return fail(FMCW_EINVAL, "prf_units[%u] %u (1..4096)", k, c.prf_units[k]);
    for (uint32_t j = 0; j < k; ++j)
      if (c.prf_units[j] == c.prf_units[k])
        return fail(FMCW_EINVAL, "prf_units[%u] and prf_units[%u] are both %u (pairwise distinct)", j, k, c.prf_units[k]);
    p_min = std::min(p_min, c.prf_units[k]);
  }
  if (c.prf_phase >= c.n_prf) return fail(FMCW_EINVAL, "prf_phase %u (0..n_prf - 1 = %u)", c.prf_phase, c.n_prf - 1);
  if (c.step < 1 || c.step > c.n_prf) return fail(FMCW_EINVAL, "step %u (1..n_prf = %u)", c.step, c.n_prf);
  if (c.zero_bin >= c.n_doppler) return fail(FMCW_EINVAL, "zero_bin %u (0..n_doppler - 1 = %u)", c.zero_bin, c.n_doppler - 1);
  const uint64_t v_lim = 32ull * c.n_doppler * p_min;
  if (c.v_max > v_lim)
    return fail(FMCW_EINVAL, "v_max %u (0..32 n_doppler min prf_units = %llu)", c.v_max, (unsigned long long)v_lim);
  if (c.out_unit < 1 || c.out_unit > 65535 || 2ull * c.v_max / c.out_unit + 1 > 65535)
    return fail(FMCW_EINVAL, "out_unit %u (1..65535, 2 v_max / out_unit + 1 <= 65535)", c.out_unit);
  if (c.m_of < 1 || c.m_of > c.n_prf) return fail(FMCW_EINVAL, "m_of %u (1..n_prf = %u)", c.m_of, c.n_prf);
  if (c.n_streams < 1 || c.n_streams > 4096) return fail(FMCW_EINVAL, "n_streams %u (1..4096)", c.n_streams);
  if (c.max_recs < 1 || (uint64_t)c.max_recs * dwells_per_record(c) > 0x7fffffffull)
    return fail(FMCW_EINVAL, "max_recs %u (>= 1, max_recs ceil(n_prf / step) < 2^31)", c.max_recs);
  if (c.max_frames < c.n_streams || c.max_frames % c.n_streams || (uint64_t)c.max_frames * c.n_prf > 0x7fffffffull)
    return fail(FMCW_EINVAL, "max_frames %u (a multiple of n_streams %u, max_frames n_prf < 2^31)", c.max_frames,
                c.n_streams);
  if (int rc = fmcw::check_device_id(c.device_id)) return rc;
  return FMCW_OK;
}

}  // namespace

struct fmcw_unfolder {
  fmcw_unfold_config cfg;
  UnfoldGeom geom;
  uint32_t grid = kMaxGrid;      // workgroups of index / find / emit at most (fmcw_unfold_set_grid_for_test)
  uint64_t* masks = nullptr;     // kGroups per tile: 1 bit per pair
  uint32_t* tile_cnt = nullptr;  // per tile: report count, then its exclusive scan
  uint32_t* tie_cnt = nullptr;   // per tile: reports with n_ties > 1
  uint32_t* folds = nullptr;     // per pair: best fold | n_ties << 16
  uint32_t* start = nullptr;     // max_frames + 1 words: the frame index
  uint32_t* vstart = nullptr;    // max_frames K + 1 words: the pair index
};

extern "C" {

void fmcw_unfold_config_default(fmcw_unfold_config* cfg) {
  if (!cfg) return;
  *cfg = fmcw_unfold_config{};
  cfg->n_range = 1024;
  cfg->n_doppler = 128;
  cfg->n_prf = 3;
  cfg->prf_units[0] = 8, cfg->prf_units[1] = 9, cfg->prf_units[2] = 10;
  cfg->prf_phase = 0;
  cfg->step = 3;
  cfg->zero_bin = 0;
  cfg->v_max = 2 * 128 * 8;
  cfg->out_unit = 8;
  cfg->tol_range = 1;
  cfg->tol_doppler = 1;
  cfg->m_of = 2;
  cfg->n_streams = 1;
  cfg->max_recs = 1u << 20;
  cfg->max_frames = 1024;
  cfg->device_id = 0;
}

int fmcw_unfold_create(const fmcw_unfold_config* cfg, fmcw_unfolder** out) {
  if (!cfg || !out) return fail(FMCW_EINVAL, "null argument");
  *out = nullptr;
  int rc = validate(*cfg);
  if (rc) return rc;
  if ((rc = fmcw::open_device(cfg->device_id))) return rc;
  fmcw_unfolder* u = new fmcw_unfolder();
  u->cfg = *cfg;
  uint64_t units[2] = {0, 0};
  for (uint32_t k = 0; k < cfg->n_prf; ++k) units[k >> 2] |= (uint64_t)cfg->prf_units[k] << (16 * (k & 3));
  u->geom = UnfoldGeom{cfg->n_range, cfg->n_doppler, cfg->n_prf, cfg->prf_phase, cfg->step, cfg->zero_bin, cfg->v_max,
                       cfg->out_unit, cfg->tol_range, cfg->tol_doppler, cfg->m_of, cfg->n_streams, units[0], units[1]};
  // tiles of max_recs ceil(K / step) pairs
  const size_t max_tiles = fmcw::tiles_of((uint64_t)cfg->max_recs * dwells_per_record(*cfg), UnfoldTiles::kTile);
  const size_t mask_bytes = max_tiles * UnfoldTiles::kGroups * sizeof(uint64_t), cnt_bytes = max_tiles * 4;
  const size_t fold_bytes = max_tiles * UnfoldTiles::kTile * 4;
  const size_t start_bytes = ((size_t)cfg->max_frames + 1) * 4, vstart_bytes = ((size_t)cfg->max_frames * cfg->n_prf + 1) * 4;
  if (!fmcw::alloc_scratch({fmcw::scratch(u->masks, mask_bytes), fmcw::scratch(u->tile_cnt, cnt_bytes),
                            fmcw::scratch(u->tie_cnt, cnt_bytes), fmcw::scratch(u->folds, fold_bytes),
                            fmcw::scratch(u->start, start_bytes), fmcw::scratch(u->vstart, vstart_bytes)})) {
    fmcw_unfold_destroy(u);
    return fail(FMCW_ENOMEM, "hipMalloc(%zu + 2 x %zu + %zu + %zu + %zu) for the unfolder's masks, tile counts, folds and indices failed",
                mask_bytes, cnt_bytes, fold_bytes, start_bytes, vstart_bytes);
  }
  *out = u;
  return FMCW_OK;
}

int fmcw_unfold_destroy(fmcw_unfolder* u) {
  if (!u) return FMCW_OK;
  fmcw::free_scratch(u->cfg.device_id, {u->masks, u->tile_cnt, u->tie_cnt, u->folds, u->start, u->vstart});
  delete u;
  return FMCW_OK;
}

int fmcw_unfold_set_grid_for_test(fmcw_unfolder* u, uint32_t grid) {
  if (!u) return fail(FMCW_EINVAL, "null unfolder");
  u->grid = fmcw::clamp_grid(grid, kMaxGrid);
  return FMCW_OK;
}

int fmcw_unfold_enqueue(fmcw_unfolder* u, const void* recs_dev, size_t rec_stride, size_t rec_cap,
                        const uint32_t* n_recs_dev, size_t n_scans, fmcw_vplot* out_dev, size_t out_cap,
                        uint32_t* status_dev, void* stream) {
  // what does not depend on the unfolder first, so that it can be checked without one
  if (int rc = fmcw::check_rec_list_args(recs_dev, rec_stride, rec_cap, n_recs_dev, out_dev, out_cap, status_dev)) return rc;
  if (!u) return fail(FMCW_EINVAL, "null unfolder");
  const fmcw_unfold_config& c = u->cfg;
  if (n_scans > c.max_frames / c.n_streams)
    return fail(FMCW_EINVAL, "n_scans %zu x n_streams %u above max_frames %u", n_scans, c.n_streams, c.max_frames);
  if (hipSetDevice(c.device_id) != hipSuccess) return fail(FMCW_EHIP, "hipSetDevice");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  // cap x ceil(K / step) pairs, < 2^31 (validate)
  const fmcw::ListPlan lp = fmcw::plan_list(rec_cap, c.max_recs, dwells_per_record(c), UnfoldTiles::kTile, u->grid);
  const uint32_t ocap = (uint32_t)std::min<size_t>(out_cap, 0x7fffffffu);   // fewer than 2^31 reports
  const uint32_t n_dwells = n_scans >= c.n_prf ? (uint32_t)((n_scans - c.n_prf) / c.step) + 1 : 0u;
  const UnfoldList l = {{static_cast<const uint8_t*>(recs_dev), (uint32_t)rec_stride, lp.cap, n_recs_dev, u->start,
                         (uint32_t)n_scans * c.n_streams},
                        u->vstart, n_dwells * c.n_streams * c.n_prf, lp.cap * dwells_per_record(c)};   // n_q <= max_frames K
  const dim3 grid(lp.grid), threads(UnfoldTiles::kThreads);
  const bool pairs = lp.tiles && l.n_q;
  if (lp.tiles) {
    hipLaunchKernelGGL((k_frame_index<UnfoldTiles::kThreads, UnfoldTiles::kPer, true>), dim3(lp.index_grid), threads, 0, s,
                       l.recs, l.stride, l.cap, l.n_recs, l.n_groups, u->start);
    if (int rc = fmcw::check_launch("k_frame_index")) return rc;
  }
  if (pairs) {
    hipLaunchKernelGGL(k_unfold_dwells, dim3(1), dim3(kScanThreads), 0, s, l, u->geom, u->vstart);
    if (int rc = fmcw::check_launch("k_unfold_dwells")) return rc;
    hipLaunchKernelGGL(k_unfold_find, grid, threads, 0, s, l, u->geom, u->masks, u->tile_cnt, u->tie_cnt, u->folds);
    if (int rc = fmcw::check_launch("k_unfold_find")) return rc;
  }
  hipLaunchKernelGGL(k_unfold_scan, dim3(1), dim3(kScanThreads), 0, s, l, u->tile_cnt, u->tie_cnt, status_dev);
  if (int rc = fmcw::check_launch("k_unfold_scan")) return rc;
  if (pairs && ocap) {
    hipLaunchKernelGGL(k_unfold_emit, grid, threads, 0, s, l, u->geom, u->masks, u->tile_cnt, u->folds, out_dev, ocap);
    if (int rc = fmcw::check_launch("k_unfold_emit")) return rc;
  }
  return FMCW_OK;
}

}  // extern "C"
