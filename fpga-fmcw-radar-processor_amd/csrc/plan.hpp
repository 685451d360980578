// plan.hpp -- the launch plan of a handle: everything that follows from fmcw_config alone (kernel
// selection, geometry, chunking, buffer sizes), decided once by build_plan and read-only after.
// No HIP call is made here; what needs the device (occupancy grids, function attributes) is
// fmcw_create's second step (fmcw_api.hip device_grids).
#pragma once
#include <algorithm>

#include "../../include/fmcw.h"
#include "dispatch.hpp"

namespace fmcw {

constexpr size_t kCfar2Batch = 16;  // frames per 2-D CFAR launch on the caller's map (at least)

// What a configuration leaves open.  The release library always takes the defaults; FMCW_LAB
// builds set them from the environment (fmcw_api.hip lab_knobs).
struct PlanPrefs {
  int k1_want = kRangePx;   // preferred K1 family (range_info's `want`)
  bool k2_generic = false;  // the generic K2 on a configuration that qualifies for FAST
};

struct Plan {
  fmcw_config cfg;
  RangeInfo k1;        // K1 of the path: writes cfg.spectrum_dtype
  RangeInfo k1_stage;  // K1 of fmcw_range_ct: the fp32 spectrum whatever spectrum_dtype; T / RB equal k1's
  DopplerInfo k2;
  bool k2_fast;        // K2 runs its FAST instantiation
  Cfar1Fn cfar1;       // stand-alone 1-D CFAR (fmcw_cfar); nullptr unless cfar_kind is OS1D
  Cfar2Info cfar2;     // zero unless cfar_kind is OS2D, as cf2
  Cfar1DArgs cf1;
  Cfar2DArgs cf2;
  int lgT, lgRB;       // log2 of k1.T / k1.RB (K2's un-tiling shifts)
  int tiles_frame;     // detection tiles per frame: K2's wave tiles (k2.WR range rows), shared by both CFARs
  int wpb;             // wave tiles per K2 / 1-D CFAR workgroup (DopplerGeom<NC>::WPB)
  size_t frame_px;           // n_range * n_doppler
  size_t in_frame_bytes;     // one frame of the input cube, all rx
  size_t frame_inter;        // one frame of the K1 -> K2 spectrum, all rx
  bool q15;            // window Q15_RTL
  float q15_scale;     // 2^-range_shift on the Q15 path (the fp32 window tables carry it otherwise)
  uint32_t chunk;      // frames per K1 -> K2 chunk
  size_t inter_bytes;  // the intermediate buffer (chunk frames of the spectrum, >= one fp32 frame)
  int k3_frames, k3_launches;  // 2-D CFAR: frames per K3 launch at most, K3 launches per call at most
  size_t n_wg_max;             // detection tiles of max_frames frames
  uint32_t slot_cap;           // detection records per tile slot (more -> overflow region)
  uint32_t ovf_base;           // first overflow record
  uint32_t det_scratch_cap;    // records of the detection scratch
};

// The configuration checks of fmcw_create, in their order (tests/kernel_matrix.py `legal` mirrors it).
int validate(const fmcw_config& c);
// Fills `p` from a configuration that passed validate(); FMCW_EINVAL where no kernel serves it.
int build_plan(const fmcw_config& c, const PlanPrefs& prefs, Plan* p);

// Steps per 2-D CFAR strip.  A strip of S steps loads S*TR + 2*hr rows for S*TR CUT rows; the
// workgroups run ceil(strips / grid) rounds.  Cost model per round, in units of one step's
// compute: S * (1 + 0.5) (a step's TR new rows cost about half its compute) + 0.5 * 2hr / TR for
// the halo rows a strip loads once.  Longer strips: less halo traffic, fewer strips to spread.
inline int cfar2_steps_model(int nf, int tpf, int grid, int tr, int hr) {
  int best = 1;
  double best_cost = 1e300;
  // S up to 64: config 5 (2048 steps per frame, 16 frames, 512 workgroups) then takes one round
  // of 64-step strips (measured 1,011 -> 976 us per launch) instead of two of 32
  for (int S = 1; S <= std::min(64, tpf); ++S) {
    const long strips = (long)nf * ((tpf + S - 1) / S);
    const long rounds = (strips + grid - 1) / std::max(1, grid);
    const double cost = (double)rounds * (1.5 * S + (double)hr / tr);
    if (cost < best_cost - 1e-9) {
      best_cost = cost;
      best = S;
    }
  }
  return best;
}

}  // namespace fmcw
