// launch.hip -- the one launch site of each kernel of the plan (K1, K2, the CFARs), and the
// device-dependent part of their set-up: the persistent grids.
#include <algorithm>

#include "handle.hpp"

namespace fmcw {
namespace {

// K3b / K3c grids (4 waves per workgroup; K3b one candidate per wave at a time, K3c one wave tile).
// Round 5, with k_cfar2d_lv's ~10^5 candidates per 16-frame launch at config 5 (tools/cfar2d_bench.py,
// profiles/r05/k3_rules/): 1024 / 256 workgroups 336 us per launch, 2048 / 256 323, 2048 / 1024
// 302, 4096 / 2048 297; with round 4's few thousand candidates the grid was measured neutral.
// After K3b's software pipeline (later in round 5; tools/k3_grid_ab.sh, profiles/r05/k3_grid/, two
// interleaved passes, us per K3 batch, config 5 / config 3): 2048 / 1024 workgroups 261, 252 /
// 75.6, 75.1; 1024 / 1024 258, 250 / 73.3, 72.3; 4096 / 1024 253, 255 / 81.7, 81.4; emit grids 256 /
// 512 within noise.  With k_cfar2d_lv's later levels (8x fewer candidates at config 5) 2048 / 1024 /
// 512 decide workgroups and emit grids 1024 / 256 all measured 222-231 us (k3grid2, noise): 1024.
constexpr int kCfar2DecideGrid = 1024;
constexpr int kCfar2EmitGrid = 1024;

template <typename F>
int occupancy_grid(F fn, int nt, size_t smem, int n_cu) {
  int per_cu = 0;
  hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void*>(fn),
                                                              nt, smem);
  if (e != hipSuccess || per_cu < 1) per_cu = 1;
  return per_cu * n_cu;
}

DetSink make_sink(const fmcw_handle* h) {
  DetSink s;
  s.scratch = h->det_scratch;
  s.cap = h->plan.det_scratch_cap;
  s.slot_cap = h->plan.slot_cap;
  s.ovf_base = h->plan.ovf_base;
  s.counter = h->counter;
  s.wg_base = h->wg_base;
  s.wg_count = h->wg_count;
  return s;
}

// The grid of a kernel that works through wave tiles (K2, the stand-alone 1-D CFAR): wpb tiles per
// workgroup, at most the persistent grid.
struct TileGrid {
  int n_tiles, grid;
};
TileGrid tile_grid(const fmcw_handle* h, int nf) {
  const int n_tiles = nf * h->plan.tiles_frame, wpb = h->plan.wpb;
  return {n_tiles, std::min((n_tiles + wpb - 1) / wpb, h->grid.doppler)};
}

}  // namespace

fmcw_grids device_grids(const Plan& p, int n_cu) {
  fmcw_grids g;
  g.range = occupancy_grid(p.k1.fn, p.k1.NT, 0, n_cu);
  g.doppler = occupancy_grid(p.k2.fn, p.k2.NT, 0, n_cu);
  if (p.cfg.cfar_kind == FMCW_CFAR_OS2D) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(p.cfar2.fn), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)p.cfar2.smem) != hipSuccess)
      (void)hipGetLastError();
    g.cfar = occupancy_grid(p.cfar2.fn, 256, p.cfar2.smem, n_cu);
  }
  g.k3b = kCfar2DecideGrid;
  g.k3c = kCfar2EmitGrid;
  return g;
}

int launch_range(fmcw_handle* h, const RangeInfo& ri, const void* src, int nf, const float* chirp_w,
                 uint32_t* status, hipStream_t s) {
  const Plan& p = h->plan;
  const int n_groups = nf * (int)p.cfg.n_rx * (int)(p.cfg.n_doppler / ri.T);
  ProfScope ps(&h->prof, FMCW_K_RANGE);
  // grid.range is the occupancy grid of the path's K1 (plan.k1).  The stage kernel (plan.k1_stage,
  // fmcw_range_ct) runs on the same grid, capped by its group count as any launch: its groups have
  // k1's size (build_plan checks T and RB), and K1 strides over the groups, so any grid is correct.
  launch_k(ps, true, ri.fn, dim3(std::min(n_groups, h->grid.range)), dim3(ri.NT), 0u, s, src, h->inter,
           (const float*)h->win_r, chirp_w, (int)p.cfg.n_doppler, n_groups, p.q15_scale, status);
  return check_launch("k_range");
}

int launch_doppler(fmcw_handle* h, int nf, size_t f0, float* lin, float* db, uint32_t* status, hipStream_t s) {
  const Plan& p = h->plan;
  const fmcw_config& c = p.cfg;
  const TileGrid tg = tile_grid(h, nf);
  ProfScope ps(&h->prof, FMCW_K_DOPPLER);
  launch_k(ps, true, p.k2.fn, dim3(tg.grid), dim3(p.k2.NT), 0u, s, (const float2*)h->inter, (const float*)h->win_d,
           (int)c.n_range, (int)c.n_rx, p.lgT, p.lgRB, tg.n_tiles, (int)f0, (int)(f0 * p.tiles_frame), lin, db,
           c.mag_mode, (c.compat_rtl & FMCW_COMPAT_MTI) ? 1 : 0, p.q15 ? 1 : 0, p.cf1, make_sink(h), status);
  return check_launch("k_doppler");
}

int launch_cfar(fmcw_handle* h, const float* map_chunk, int nf, int frame0, hipStream_t s) {
  const Plan& p = h->plan;
  const fmcw_config& c = p.cfg;
  const DetSink sink = make_sink(h);
  const int tile0 = frame0 * p.tiles_frame;
  if (c.cfar_kind == FMCW_CFAR_OS2D) {
    const Cfar2DArgs& a = p.cf2;
    const Cfar2Info& ci = p.cfar2;
    // pieces of at most k3_frames frames (the candidate lists' capacity), each its own K3a/b/c
    for (int p0 = 0; p0 < nf; p0 += p.k3_frames) {
      const int np = std::min(p.k3_frames, nf - p0);
      if (h->k3_launch_idx >= p.k3_launches) return fail(FMCW_EINVAL, "2-D CFAR: launch counter slots exhausted");
      Cfar2Cands cands{h->cand_cell, h->cand_thr, h->cand_tiles, h->k3_ctr + 2 * h->k3_launch_idx++,
                       h->cand_pcell, h->cand_ptile};
      const float* mp = map_chunk + (size_t)p0 * p.frame_px;
      // workgroup tiles (steps): 4 consecutive wave tiles of one frame; a strip is `steps` of them
      const int tpf = (p.tiles_frame + 3) / 4;
      const int steps = h->cfar2_steps ? std::min(h->cfar2_steps, tpf)
                                       : cfar2_steps_model(np, tpf, h->grid.cfar, p.k2.WR * 4, a.hr);
      const int n_strips = np * ((tpf + steps - 1) / steps);
      const int grid = std::min(n_strips, h->grid.cfar);
      h->cfar2_steps_last = steps;
      ProfScope ps(&h->prof, FMCW_K_CFAR2D);
      launch_k(ps, false, ci.fn, dim3(grid), dim3(256), (uint32_t)ci.smem, s, mp, (int)c.n_range, n_strips, steps,
               frame0 + p0, tile0 + p0 * p.tiles_frame, a, sink, cands);
      if (int rc = check_launch("k_cfar2d")) return rc;
      // K3b / K3c: fixed grids that read the candidate counts on the device (no host round trip)
      launch_k(ps, false, ci.decide, dim3(h->grid.k3b), dim3(256), 0u, s, mp, (int)c.n_range, a, cands);
      launch_k(ps, true, ci.emit, dim3(h->grid.k3c), dim3(256), 0u, s, mp, (int)c.n_range, frame0 + p0, a, cands,
               sink);
      if (int rc = check_launch("k_cfar2d_decide / _emit")) return rc;
    }
    return FMCW_OK;
  }
  // 1-D on a caller map (fmcw_cfar); inside fmcw_enqueue the 1-D CFAR is fused into K2
  const TileGrid tg = tile_grid(h, nf);
  ProfScope ps(&h->prof, FMCW_K_CFAR2D);
  launch_k(ps, true, p.cfar1, dim3(tg.grid), dim3(p.k2.NT), 0u, s, map_chunk, (int)c.n_range, tg.n_tiles, frame0,
           tile0, p.cf1, sink);
  return check_launch("k_cfar1d");
}

}  // namespace fmcw
