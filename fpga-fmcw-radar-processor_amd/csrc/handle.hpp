// handle.hpp -- fmcw_handle: the plan (read-only after fmcw_create), the device buffers it sized,
// per-call state and the profiler; and the host functions of the other translation units that
// work on it.
#pragma once
#include "internal.hpp"
#include "plan.hpp"
#include "profiling.hpp"

// The persistent grids: workgroups the device holds at once (occupancy x CUs), computed at
// fmcw_create; fmcw_set_param (FMCW_PARAM_GRID_*) can cap each below its created value.
struct fmcw_grids {
  int range = 0, doppler = 0, cfar = 0;  // K1, K2 (and the stand-alone 1-D CFAR), K3a
  int k3b = 0, k3c = 0;                  // K3b / K3c (kCfar2DecideGrid / kCfar2EmitGrid)
};

struct fmcw_handle {
  const fmcw::Plan plan;
  const fmcw_grids grid_created;  // as fmcw_create computed them
  fmcw_grids grid;                // the launches' bounds: min(created, FMCW_PARAM_GRID_* cap)
  // device buffers
  float* win_r = nullptr;  // [ns]
  float* win_d = nullptr;  // [nc]
  float2* inter = nullptr; // plan.inter_bytes: chunk frames of the K1 -> K2 spectrum
  float* lin_scratch = nullptr;  // chunk * ns * nc (2-D CFAR input when the caller wants no linear map)
  fmcw_det* det_scratch = nullptr;
  uint32_t* counter = nullptr;  // [0] overflow entries used, [1] dropped
  uint32_t* sat = nullptr;      // [0] window, [1] word saturations of the current call (status words 2, 3)
  // the per-call device counters (counter[0..1], sat, k3_ctr) are zero: re-armed by the previous
  // call's k_det_list (or at fmcw_create); a call that stopped early leaves this false and the
  // next one zeroes them first
  bool counters_armed = false;
  uint32_t* wg_base = nullptr;
  uint32_t* wg_count = nullptr;
  uint64_t* lb_status = nullptr;  // k_det_list look-back words (det_lb_words of them)
  uint32_t* det_epoch = nullptr;   // k_det_list's device-resident call tag and publish count (2 words)
  uint32_t* n_dets_tmp = nullptr;
  // fmcw_process host-copy staging, grown on demand and kept (no allocator call per frame batch)
  void* stage_cube = nullptr;
  size_t stage_cube_bytes = 0;
  float* stage_map = nullptr;
  size_t stage_map_bytes = 0;
  fmcw_det* stage_dets = nullptr;
  size_t stage_dets_cap = 0;
  int cfar2_steps = 0;                  // 2-D CFAR steps per strip (0 = cost model; FMCW_PARAM_CFAR2D_STEPS)
  int cfar2_steps_last = 0;             // the strip length of the last 2-D CFAR launch (FMCW_INFO_CFAR2D_STEPS)
  // 2-D CFAR candidate lists (kernel_types.hpp Cfar2Cands): room for every cell of plan.k3_frames frames,
  // and a counter pair per K3 launch of a call (plan.k3_launches of them, zeroed with the status words)
  uint32_t* cand_cell = nullptr;
  float* cand_thr = nullptr;
  uint32_t* cand_tiles = nullptr;
  uint32_t* cand_pcell = nullptr;   // k_cfar2d_lv's strip-private spill regions (Cfar2Cands pcell / ptile)
  uint32_t* cand_ptile = nullptr;
  uint32_t* k3_ctr = nullptr;
  int k3_launch_idx = 0;                // launches of the current call so far
  uint32_t last_status[2] = {0, 0};     // fmcw_process: status words 2, 3 of its last call
  fmcw::Profiler prof;

  fmcw_handle(const fmcw::Plan& p, const fmcw_grids& g) : plan(p), grid_created(g), grid(g) {}
};

namespace fmcw {

// ---- the plan's kernels (launch.hip) -----------------------------------------------------------
// fmcw_create's second step, the part of the set-up that needs the device: the occupancy grids of
// the plan's kernels on n_cu compute units (and K3a's dynamic-LDS attribute)
fmcw_grids device_grids(const Plan& p, int n_cu);
// K1 `ri` (plan.k1 or plan.k1_stage) on nf frames at src -> h->inter; chirp_w: the Doppler window
// fused into K1, or nullptr; status: saturation counters, or nullptr
int launch_range(fmcw_handle* h, const RangeInfo& ri, const void* src, int nf, const float* chirp_w,
                 uint32_t* status, hipStream_t s);
// K2 on the nf frames in h->inter, frames f0 .. of the call -> lin / db maps (either may be null)
int launch_doppler(fmcw_handle* h, int nf, size_t f0, float* lin, float* db, uint32_t* status, hipStream_t s);
// The CFAR on nf frames of a linear map, shared by fmcw_enqueue (2-D: the map K2 just produced)
// and fmcw_cfar: K3a/b/c, or the stand-alone 1-D kernel
int launch_cfar(fmcw_handle* h, const float* map_chunk, int nf, int frame0, hipStream_t s);

// ---- detection list (detlist.hip) ----------------------------------------------------------
// look-back words k_det_list needs for n_tiles detection tiles (one per workgroup)
size_t det_lb_words(size_t n_tiles);
// zeroes n words at `w` on the stream (the caller's status words of a call without a CFAR)
int zero_words(uint32_t* w, int n, hipStream_t s);
// Zero the per-call counters unless the previous call's k_det_list left them armed; `cap`: the
// stream is being captured into a graph.
int arm_counters(fmcw_handle* h, hipStream_t s, bool cap);
// k_det_list over the tiles of n_frames frames: the ordered list, the status words, the re-arming
int launch_det_finish(fmcw_handle* h, size_t n_frames, fmcw_det* dets, size_t det_cap, uint32_t* n_dets_dev,
                      uint32_t* sat, hipStream_t s);

// ---- stage kernels (stage_kernels.hip) -------------------------------------------------------
// inter (K1 tiles of T chirps x RB range bins) -> spec[fr][r][c], `total` points
int launch_unblock(const float2* inter, float2* spec, int ns, int nc, int T, int RB, size_t total, hipStream_t s);
int launch_magnitude(const float2* iq, float* out, size_t n, int mode, hipStream_t s);

}  // namespace fmcw
