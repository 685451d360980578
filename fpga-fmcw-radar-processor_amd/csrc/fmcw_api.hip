// fmcw_api.hip -- the C-ABI of libfmcw.so declared in include/fmcw.h: the entry points.
//
// The handle replaces the reference's elaborated radar_core instance (rtl/src/radar_core.vhd
// generics :12-19, FFT IP configuration handshake cfg_proc :279-301): fmcw_create validates the
// configuration and builds the launch plan once (plan.hip), uploads the window tables
// (window_multiplier.vhd:34-49, as fp32) and allocates every scratch buffer, so fmcw_enqueue only
// launches kernels (launch.hip, detlist.hip; graph-capturable).
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "handle.hpp"

using namespace fmcw;

namespace fmcw {

thread_local std::string g_err;  // fmcw_last_error() of the calling thread

int fail(int code, const char* fmt, ...) {
  char b[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(b, sizeof b, fmt, ap);
  va_end(ap);
  g_err = b;
  return code;
}

int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(FMCW_EHIP, "launch %s: %s", what, hipGetErrorString(e));
  return FMCW_OK;
}

// fp32 window table: Hamming with the RTL's half-ROM mirrored address, computed in fp64
// (window_multiplier.vhd:34-49, :97-102).  WIN_NONE uploads ones.
std::vector<float> window_table(uint32_t n, int kind, uint32_t shift) {
  std::vector<float> w(n, std::ldexp(1.0f, -(int)shift));  // 2^-shift: exact
  if (kind != FMCW_WIN_Q15_RTL && kind != FMCW_WIN_HAMMING) return w;
  const uint32_t half = n / 2;
  for (uint32_t i = 0; i < n; ++i) {
    uint32_t a = i < half ? i : n - 1 - i;
    if (a > half - 1) a = half - 1;
    const double wa = 0.54 - 0.46 * std::cos(2.0 * M_PI * (double)a / (double)(n - 1));
    // Q15: the ROM integers c = integer(w * 32767) (:43-46), mirrored
    w[i] = kind == FMCW_WIN_Q15_RTL ? (float)std::min(32767.0, std::floor(wa * 32767.0 + 0.5))
                                    : std::ldexp((float)wa, -(int)shift);
  }
  return w;
}

}  // namespace fmcw

namespace {

// The A/B knobs of FMCW_LAB builds (tools/build_variants.sh), read from the environment once per
// fmcw_create, after the release plan and grids exist; the release library reads no environment.
//   FMCW_K1=single|seq|px, FMCW_K2_GENERIC: another kernel selection -- plan and grids are built again
//   FMCW_CFAR2D_STEPS: the handle's initial FMCW_PARAM_CFAR2D_STEPS
//   FMCW_GRID_RANGE / _DOPPLER / _CFAR: cap a persistent grid so that another stream's kernels
//   find free CU slots beside it (tools/overlap_lab.py); FMCW_GRID_K3B / _K3C: set the fixed grids
int lab_knobs(int n_cu, Plan* plan, fmcw_grids* g, int* cfar2_steps) {
#if FMCW_LAB
  PlanPrefs prefs;
  if (const char* k1 = std::getenv("FMCW_K1"))
    prefs.k1_want = !std::strcmp(k1, "single") ? kRangeSingle : !std::strcmp(k1, "seq") ? kRangeSeq : kRangePx;
  prefs.k2_generic = std::getenv("FMCW_K2_GENERIC") != nullptr;
  if (prefs.k1_want != kRangePx || prefs.k2_generic) {
    const fmcw_config c = plan->cfg;
    if (int rc = build_plan(c, prefs, plan)) return rc;
    *g = device_grids(*plan, n_cu);
  }
  if (const char* cs = std::getenv("FMCW_CFAR2D_STEPS")) *cfar2_steps = std::max(0, std::atoi(cs));
  auto knob = [](const char* name) {
    const char* v = std::getenv(name);
    return v ? std::atoi(v) : 0;
  };
  for (auto [name, grid] : {std::pair<const char*, int*>{"FMCW_GRID_RANGE", &g->range},
                            {"FMCW_GRID_DOPPLER", &g->doppler}, {"FMCW_GRID_CFAR", &g->cfar}})
    if (const int n = knob(name); n > 0) *grid = std::min(*grid, n);
  for (auto [name, grid] : {std::pair<const char*, int*>{"FMCW_GRID_K3B", &g->k3b}, {"FMCW_GRID_K3C", &g->k3c}})
    if (const int n = knob(name); n > 0) *grid = n;
#endif
  return FMCW_OK;
}

// true while `s` is being captured into a hipGraph (nothing the call enqueues runs now)
bool capturing(hipStream_t s) {
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(s, &st) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return st == hipStreamCaptureStatusActive;
}

bool is_device_ptr(const void* p) {
  if (!p) return false;
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeManaged;
}

// Grow-only device staging owned by the handle (fmcw_process with host buffers).
template <typename T>
int ensure_stage(T** p, size_t* have, size_t need_bytes, const char* what) {
  if (*have >= need_bytes) return FMCW_OK;
  if (*p) hipFree(*p);
  *p = nullptr;
  *have = 0;
  if (hipMalloc(reinterpret_cast<void**>(p), need_bytes) != hipSuccess) {
    (void)hipGetLastError();
    return fail(FMCW_ENOMEM, "hipMalloc(%zu) for the %s staging buffer failed", need_bytes, what);
  }
  *have = need_bytes;
  return FMCW_OK;
}

}  // namespace

// =======================================================================================
extern "C" {

const char* fmcw_version(void) { return "fmcw-mi355x 0.1.0 (gfx950)"; }
int fmcw_abi_version(void) { return FMCW_ABI_VERSION; }
const char* fmcw_last_error(void) { return g_err.c_str(); }

void fmcw_config_default(fmcw_config* c) {
  if (!c) return;
  std::memset(c, 0, sizeof *c);
  c->n_range = 1024;  // radar_core.vhd:13
  c->n_doppler = 128; // :14
  c->n_rx = 1;
  c->in_dtype = FMCW_IN_F32;
  c->window = FMCW_WIN_HAMMING;
  c->mag_mode = FMCW_MAG_ABS;
  c->map_kind = FMCW_MAP_LINEAR;
  c->cfar_kind = FMCW_CFAR_OS2D;
  c->cfar1d_ref = 8;  // rtl/old/radar_core_v3.vhd:376-380
  c->cfar1d_guard = 2;
  c->cfar1d_rank = 12;
  c->cfar1d_alpha = 4.0f;
  c->cfar2d_ref_range = 4;     // radar_core.vhd:16 CFAR_REF_R (rows)
  c->cfar2d_guard_range = 1;   // :19 CFAR_GUARD_D=1 acts on rows (naming swap)
  c->cfar2d_ref_doppler = 4;   // :17 CFAR_REF_D
  c->cfar2d_guard_doppler = 2; // :18 CFAR_GUARD_R=2 acts along Doppler
  c->cfar2d_rank_pct = 75;     // :380
  c->cfar2d_scale_min = 2;
  c->cfar2d_scale_nom = 4;
  c->cfar2d_scale_max = 6;
  c->cfar2d_scale_override = 0;
  c->max_frames = 1;
  c->chunk_frames = 0;
  c->device_id = 0;
}

int fmcw_create(const fmcw_config* cfg, fmcw_handle** out) {
  if (!cfg || !out) return fail(FMCW_EINVAL, "null argument");
  *out = nullptr;
  int rc = validate(*cfg);
  if (rc) return rc;
  // not open_device(): validate() leaves device_id to this sequence (a negative one is FMCW_ENODEV
  // here), and a device that cannot be selected or queried is FMCW_EHIP with the HIP error's text
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) {
    (void)hipGetLastError();
    return fail(FMCW_ENODEV, "no HIP device");
  }
  if (cfg->device_id < 0 || cfg->device_id >= ndev) return fail(FMCW_ENODEV, "device_id %d out of range", cfg->device_id);
  HIP_TRY(hipSetDevice(cfg->device_id));
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, cfg->device_id));
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(FMCW_ENODEV, "device %d is %s; this build targets gfx950 (MI355X)", cfg->device_id,
                prop.gcnArchName);

  // the plan (configuration alone), then what of it needs the device
  Plan plan;
  if ((rc = build_plan(*cfg, PlanPrefs{}, &plan))) return rc;
  fmcw_grids grids = device_grids(plan, prop.multiProcessorCount);
  int cfar2_steps = 0;
  if ((rc = lab_knobs(prop.multiProcessorCount, &plan, &grids, &cfar2_steps))) return rc;
  fmcw_handle* h = new fmcw_handle(plan, grids);
  h->cfar2_steps = cfar2_steps;
  const Plan& p = h->plan;
  const fmcw_config& c = p.cfg;
  auto cleanup = [&](int code) {
    fmcw_destroy(h);
    return code;
  };
#define ALLOC(ptr, bytes)                                                                   \
  do {                                                                                      \
    if (hipMalloc(reinterpret_cast<void**>(&(ptr)), (bytes)) != hipSuccess) {               \
      (void)hipGetLastError();                                                              \
      return cleanup(fail(FMCW_ENOMEM, "hipMalloc(%zu) for %s failed", (size_t)(bytes), #ptr)); \
    }                                                                                       \
  } while (0)
  ALLOC(h->win_r, c.n_range * sizeof(float));
  ALLOC(h->win_d, c.n_doppler * sizeof(float));
  ALLOC(h->inter, p.inter_bytes);
  if (c.cfar_kind == FMCW_CFAR_OS2D) {
    ALLOC(h->lin_scratch, p.chunk * p.frame_px * sizeof(float));
    const size_t cells = p.k3_frames * p.frame_px, tiles = (size_t)p.k3_frames * p.tiles_frame;
    ALLOC(h->cand_cell, cells * sizeof(uint32_t));
    ALLOC(h->cand_thr, cells * sizeof(float));
    ALLOC(h->cand_tiles, tiles * sizeof(uint32_t));
    if (p.cfar2.spill) {
      ALLOC(h->cand_pcell, cells * sizeof(uint32_t));
      ALLOC(h->cand_ptile, tiles * 2 * sizeof(uint32_t));
    }
    ALLOC(h->k3_ctr, (size_t)2 * p.k3_launches * sizeof(uint32_t));
  }
  const size_t lb_bytes = det_lb_words(p.n_wg_max) * sizeof(uint64_t);
  ALLOC(h->det_scratch, (size_t)p.det_scratch_cap * sizeof(fmcw_det));
  ALLOC(h->counter, 16);
  ALLOC(h->sat, 8);
  ALLOC(h->n_dets_tmp, 16);
  ALLOC(h->wg_base, p.n_wg_max * sizeof(uint32_t));
  ALLOC(h->wg_count, p.n_wg_max * sizeof(uint32_t));
  ALLOC(h->lb_status, lb_bytes);
  ALLOC(h->det_epoch, 2 * sizeof(uint32_t));
#undef ALLOC
  static const uint32_t kEpoch0[2] = {1u, 0u};  // first epoch 1 (the look-back words start at 0)
  // the range table carries the 2^-range_shift scaling (Q15: applied after the integer window)
  std::vector<float> wr = window_table(c.n_range, c.window, p.q15 ? 0 : c.range_shift),
                     wd = window_table(c.n_doppler, c.window);  // Q15: the ROM integers, applied by K2
  if (hipMemcpy(h->win_r, wr.data(), wr.size() * 4, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(h->win_d, wd.data(), wd.size() * 4, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemset(h->wg_count, 0, p.n_wg_max * sizeof(uint32_t)) != hipSuccess ||
      hipMemset(h->lb_status, 0, lb_bytes) != hipSuccess ||
      hipMemcpy(h->det_epoch, kEpoch0, sizeof kEpoch0, hipMemcpyHostToDevice) != hipSuccess)
    return cleanup(fail(FMCW_EHIP, "window upload failed"));
  *out = h;
  return FMCW_OK;
}

int fmcw_destroy(fmcw_handle* h) {
  if (!h) return FMCW_OK;
  hipSetDevice(h->plan.cfg.device_id);
  void* ptrs[] = {h->win_r, h->win_d, h->inter, h->lin_scratch, h->det_scratch, h->counter, h->sat,
                  h->n_dets_tmp, h->wg_base, h->wg_count, h->lb_status, h->det_epoch,
                  h->stage_cube, h->stage_map, h->stage_dets, h->cand_cell, h->cand_thr,
                  h->cand_tiles, h->cand_pcell, h->cand_ptile, h->k3_ctr};
  for (void* p : ptrs)
    if (p) hipFree(p);
  h->prof.destroy_events();
  delete h;
  return FMCW_OK;
}

int fmcw_enqueue(fmcw_handle* h, const void* cube, size_t n_frames, float* rd_map, fmcw_det* dets,
                 size_t det_cap, uint32_t* n_dets_dev, void* stream) {
  if (!h || !cube) return fail(FMCW_EINVAL, "null handle or cube");
  const Plan& p = h->plan;
  const fmcw_config& c = p.cfg;
  if (n_frames < 1 || n_frames > c.max_frames)
    return fail(FMCW_EINVAL, "n_frames=%zu outside [1, max_frames=%u]", n_frames, c.max_frames);
  if (c.cfar_kind != FMCW_CFAR_NONE && !n_dets_dev)
    return fail(FMCW_EINVAL, "n_dets_dev is required when a CFAR is configured");
  HIP_TRY(hipSetDevice(c.device_id));
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  // status words 2 / 3 (saturations) are counted atomically by the kernels that can saturate: into
  // the handle's `sat` words, which the call's last kernel (k_det_list) reports and re-arms
  // with the other per-call counters; without a CFAR there is no such kernel, and the caller's
  // words are zeroed and counted into directly
  const bool cfar = c.cfar_kind != FMCW_CFAR_NONE;
  uint32_t* const status = cfar ? h->sat : n_dets_dev ? n_dets_dev + 2 : nullptr;
  int rc;
  if (!cfar && n_dets_dev && (rc = zero_words(n_dets_dev, FMCW_STATUS_WORDS, s))) return rc;
  const bool cap = capturing(s);
  if (cap && h->prof.on) return fail(FMCW_EINVAL, "profiling events cannot be captured into a graph");
  if (cfar && (rc = arm_counters(h, s, cap))) return rc;
  h->k3_launch_idx = 0;
  // MTI off, fp32 window: K1 applies the Doppler window too (FFT linearity; K2 then skips
  // it); with MTI or the RTL-compat integer window K2 applies it after the canceller
  const float* chirp_w = c.mti_mode == FMCW_MTI_OFF && !p.q15 ? h->win_d : nullptr;
  const bool map_lin = rd_map && c.map_kind == FMCW_MAP_LINEAR;

  // Chunks of plan.chunk frames: K1 -> corner-turned spectrum -> K2 (+ K3)
  size_t k3_f0 = 0;  // first frame of the caller's map not yet through the 2-D CFAR
  for (size_t f0 = 0; f0 < n_frames; f0 += p.chunk) {
    // (Measured and dropped: the same number of chunks balanced in whole K2 rounds -- config 5's
    // 16 frames as 3,3,3,3,2,2 instead of 3,3,3,3,3,1: K2 59 -> 61 us per launch, configs 3 / 5
    // 1 % slower, profiles/r03/s2/ab_c*_b*.log.)
    const int nf = (int)std::min<size_t>(p.chunk, n_frames - f0);
    const void* src = static_cast<const char*>(cube) + f0 * p.in_frame_bytes;
    if ((rc = launch_range(h, p.k1, src, nf, chirp_w, status, s))) return rc;
    float* lin = map_lin ? rd_map + f0 * p.frame_px : nullptr;
    float* db = rd_map && c.map_kind == FMCW_MAP_DB ? rd_map + f0 * p.frame_px : nullptr;
    if (c.cfar_kind == FMCW_CFAR_OS2D && !lin) lin = h->lin_scratch;
    if ((rc = launch_doppler(h, nf, f0, lin, db, status, s))) return rc;
    if (c.cfar_kind == FMCW_CFAR_OS2D) {
      // on the caller's map the 2-D CFAR runs over batches of >= kCfar2Batch frames: its
      // strips then cover more rows per workgroup and more frames share one launch
      const size_t done = f0 + (size_t)nf;
      if (!map_lin) {  // chunk scratch: this chunk only
        if ((rc = launch_cfar(h, lin, nf, (int)f0, s))) return rc;
      } else if (done - k3_f0 >= kCfar2Batch || done == n_frames) {
        if ((rc = launch_cfar(h, rd_map + k3_f0 * p.frame_px, (int)(done - k3_f0), (int)k3_f0, s))) return rc;
        k3_f0 = done;
      }
    }
  }
  if (cfar) {
    if ((rc = launch_det_finish(h, n_frames, dets, det_cap, n_dets_dev, h->sat, s))) return rc;
    if (!cap) h->counters_armed = true;  // k_det_list re-arms them on the device, in stream order
  }
  return FMCW_OK;
}

int fmcw_process(fmcw_handle* h, const void* cube, size_t n_frames, float* rd_map, fmcw_det* dets,
                 size_t det_cap, size_t* n_dets, void* stream) {
  if (!h || !cube) return fail(FMCW_EINVAL, "null handle or cube");
  const Plan& p = h->plan;
  const fmcw_config& c = p.cfg;
  if (n_frames < 1 || n_frames > c.max_frames)
    return fail(FMCW_EINVAL, "n_frames=%zu outside [1, max_frames=%u]", n_frames, c.max_frames);
  HIP_TRY(hipSetDevice(c.device_id));
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const size_t cb = n_frames * p.in_frame_bytes;
  const size_t map_bytes = n_frames * p.frame_px * sizeof(float);
  const void* d_cube = cube;
  float* d_map = rd_map;
  fmcw_det* d_dets = dets;
  int rc;
  if (!is_device_ptr(cube)) {
    if ((rc = ensure_stage(&h->stage_cube, &h->stage_cube_bytes, cb, "cube"))) return rc;
    HIP_TRY(hipMemcpyAsync(h->stage_cube, cube, cb, hipMemcpyHostToDevice, s));
    d_cube = h->stage_cube;
  }
  if (rd_map && !is_device_ptr(rd_map)) {
    if ((rc = ensure_stage(&h->stage_map, &h->stage_map_bytes, map_bytes, "map"))) return rc;
    d_map = h->stage_map;
  }
  if (dets && det_cap && !is_device_ptr(dets)) {
    size_t have = h->stage_dets_cap * sizeof(fmcw_det);
    if ((rc = ensure_stage(&h->stage_dets, &have, det_cap * sizeof(fmcw_det), "detection"))) return rc;
    h->stage_dets_cap = have / sizeof(fmcw_det);
    d_dets = h->stage_dets;
  }
  if ((rc = fmcw_enqueue(h, d_cube, n_frames, d_map, d_dets, det_cap, h->n_dets_tmp, stream))) return rc;
  uint32_t ndd[FMCW_STATUS_WORDS] = {0, 0, 0, 0};  // found, dropped, window / word saturations
  hipError_t e = hipMemcpyAsync(ndd, h->n_dets_tmp, sizeof ndd, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess && rd_map && d_map != rd_map)
    e = hipMemcpyAsync(rd_map, d_map, map_bytes, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  h->last_status[0] = ndd[2];
  h->last_status[1] = ndd[3];
  const uint32_t nd = ndd[0];
  if (e == hipSuccess && dets && d_dets != dets && nd)
    e = hipMemcpy(dets, d_dets, std::min<size_t>(nd, det_cap) * sizeof(fmcw_det), hipMemcpyDeviceToHost);
  if (e != hipSuccess) return fail(FMCW_EHIP, "fmcw_process: %s", hipGetErrorString(e));
  if (n_dets) *n_dets = nd;
  if (c.cfar_kind != FMCW_CFAR_NONE && (nd > det_cap || ndd[1] > 0))
    return fail(FMCW_EDETCAP, "%u detections, det_cap %zu, %u beyond the handle's scratch", nd, det_cap,
                ndd[1]);
  return FMCW_OK;
}

int fmcw_range_ct(fmcw_handle* h, const void* cube, size_t n_frames, void* spec, void* stream) {
  if (!h || !cube || !spec) return fail(FMCW_EINVAL, "null argument");
  const Plan& p = h->plan;
  const fmcw_config& c = p.cfg;
  if (n_frames < 1 || n_frames > c.max_frames) return fail(FMCW_EINVAL, "n_frames out of range");
  HIP_TRY(hipSetDevice(c.device_id));
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  // the stage output is the fp32 spectrum whatever spectrum_dtype the path uses: plan.k1_stage, as
  // many frames per launch as the intermediate buffer holds at 8 B per point, no fused Doppler
  // window; un-tiled with the path K1's tile geometry (build_plan checks that the two agree)
  const size_t fr_px = c.n_rx * p.frame_px;
  const size_t rc_chunk = std::max<size_t>(1, p.inter_bytes / (fr_px * sizeof(float2)));
  for (size_t f0 = 0; f0 < n_frames; f0 += rc_chunk) {
    const int nf = (int)std::min<size_t>(rc_chunk, n_frames - f0);
    int rc = launch_range(h, p.k1_stage, static_cast<const char*>(cube) + f0 * p.in_frame_bytes, nf, nullptr, nullptr, s);
    if (rc) return rc;
    rc = launch_unblock(h->inter, static_cast<float2*>(spec) + f0 * fr_px, (int)c.n_range, (int)c.n_doppler, p.k1.T,
                        p.k1.RB, (size_t)nf * fr_px, s);
    if (rc) return rc;
  }
  return FMCW_OK;
}

int fmcw_magnitude(const float* iq, float* out, size_t n, int mag_mode, void* stream) {
  if (!iq || !out) return fail(FMCW_EINVAL, "null argument");
  if (mag_mode != FMCW_MAG_ABS && mag_mode != FMCW_MAG_AMBM) return fail(FMCW_EINVAL, "mag_mode");
  if (!n) return FMCW_OK;
  return launch_magnitude(reinterpret_cast<const float2*>(iq), out, n, mag_mode, reinterpret_cast<hipStream_t>(stream));
}

int fmcw_cfar(fmcw_handle* h, const float* map, size_t n_frames, fmcw_det* dets, size_t det_cap,
              uint32_t* n_dets_dev, void* stream) {
  if (!h || !map || !n_dets_dev) return fail(FMCW_EINVAL, "null argument");
  const fmcw_config& c = h->plan.cfg;
  if (c.cfar_kind == FMCW_CFAR_NONE) return fail(FMCW_EINVAL, "handle has cfar_kind NONE");
  if (n_frames < 1 || n_frames > c.max_frames) return fail(FMCW_EINVAL, "n_frames out of range");
  HIP_TRY(hipSetDevice(c.device_id));
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const bool cap = capturing(s);
  if (cap && h->prof.on) return fail(FMCW_EINVAL, "profiling events cannot be captured into a graph");
  if (int rc0 = arm_counters(h, s, cap)) return rc0;
  h->k3_launch_idx = 0;
  int rc = launch_cfar(h, map, (int)n_frames, 0, s);
  if (rc) return rc;
  if ((rc = launch_det_finish(h, n_frames, dets, det_cap, n_dets_dev, nullptr, s))) return rc;
  if (!cap) h->counters_armed = true;
  return FMCW_OK;
}

int fmcw_set_profiling(fmcw_handle* h, int enable) {
  if (!h) return fail(FMCW_EINVAL, "null handle");
  h->prof.on = enable != 0;
  return FMCW_OK;
}

namespace {

// FMCW_PARAM_GRID_* / FMCW_INFO_GRID_*: the fmcw_grids field of a key, or nullptr
struct GridKey {
  int param, info;
  const char* name;
  int fmcw_grids::*field;
};
constexpr GridKey kGridKeys[] = {
    {FMCW_PARAM_GRID_RANGE, FMCW_INFO_GRID_RANGE, "grid_range", &fmcw_grids::range},
    {FMCW_PARAM_GRID_DOPPLER, FMCW_INFO_GRID_DOPPLER, "grid_doppler", &fmcw_grids::doppler},
    {FMCW_PARAM_GRID_CFAR2D, FMCW_INFO_GRID_CFAR2D, "grid_cfar2d", &fmcw_grids::cfar},
    {FMCW_PARAM_GRID_K3B, FMCW_INFO_GRID_K3B, "grid_k3b", &fmcw_grids::k3b},
    {FMCW_PARAM_GRID_K3C, FMCW_INFO_GRID_K3C, "grid_k3c", &fmcw_grids::k3c},
};

}  // namespace

// The key and the value are checked before the handle, so the reject ranges hold without a device.
int fmcw_set_param(fmcw_handle* h, int key, int64_t value) {
  if (key == FMCW_PARAM_CFAR2D_STEPS) {
    if (value < 0 || value > (1 << 20)) return fail(FMCW_EINVAL, "cfar2d steps %lld (0 = cost model)", (long long)value);
    if (!h) return fail(FMCW_EINVAL, "null handle");
    h->cfar2_steps = (int)value;
    return FMCW_OK;
  }
  for (const GridKey& k : kGridKeys) {
    if (key != k.param) continue;
    if (value < 0 || value > (1 << 20))
      return fail(FMCW_EINVAL, "%s %lld (0 = the created grid, 1..2^20 = a cap)", k.name, (long long)value);
    if (!h) return fail(FMCW_EINVAL, "null handle");
    const int created = h->grid_created.*k.field;
    h->grid.*k.field = value ? std::min(created, (int)value) : created;
    return FMCW_OK;
  }
  if (!h) return fail(FMCW_EINVAL, "null handle");
  return fail(FMCW_EINVAL, "fmcw_set_param: unknown key %d", key);
}

int fmcw_get_info(fmcw_handle* h, int key, int64_t* value) {
  if (!h || !value) return fail(FMCW_EINVAL, "null argument");
  switch (key) {
    case FMCW_INFO_CHUNK: *value = h->plan.chunk; return FMCW_OK;
    case FMCW_INFO_RANGE_KERNEL: *value = h->plan.k1.kind; return FMCW_OK;
    case FMCW_INFO_WINDOW_SATURATIONS: *value = h->last_status[0]; return FMCW_OK;
    case FMCW_INFO_WORD_SATURATIONS: *value = h->last_status[1]; return FMCW_OK;
    case FMCW_INFO_CFAR2D_STEPS: *value = h->cfar2_steps_last; return FMCW_OK;
  }
  for (const GridKey& k : kGridKeys)
    if (key == k.info) {
      *value = h->grid.*k.field;
      return FMCW_OK;
    }
  return fail(FMCW_EINVAL, "fmcw_get_info: unknown key %d", key);
}

int fmcw_kernel_times(fmcw_handle* h, double* ms, uint64_t* launches) {
  if (!h) return fail(FMCW_EINVAL, "null handle");
  HIP_TRY(hipSetDevice(h->plan.cfg.device_id));
  if (int rc = h->prof.collect()) return rc;
  for (int k = 0; k < FMCW_K_COUNT; ++k) {
    if (ms) ms[k] = h->prof.ms[k];
    if (launches) launches[k] = h->prof.launches[k];
  }
  return FMCW_OK;
}

int fmcw_reset_kernel_times(fmcw_handle* h) {
  if (!h) return fail(FMCW_EINVAL, "null handle");
  int rc = fmcw_kernel_times(h, nullptr, nullptr);
  for (int k = 0; k < FMCW_K_COUNT; ++k) {
    h->prof.ms[k] = 0;
    h->prof.launches[k] = 0;
  }
  return rc;
}

int fmcw_device_alloc(size_t bytes, void** ptr, int device_id) {
  if (!ptr) return fail(FMCW_EINVAL, "null ptr");
  HIP_TRY(hipSetDevice(device_id));
  if (hipMalloc(ptr, bytes) != hipSuccess) {
    (void)hipGetLastError();
    return fail(FMCW_ENOMEM, "hipMalloc(%zu)", bytes);
  }
  return FMCW_OK;
}

int fmcw_device_free(void* ptr) {
  if (ptr) HIP_TRY(hipFree(ptr));
  return FMCW_OK;
}

int fmcw_memcpy(void* dst, const void* src, size_t bytes, int kind) {
  const hipMemcpyKind k = kind == 0 ? hipMemcpyHostToDevice : kind == 1 ? hipMemcpyDeviceToHost
                                                                        : hipMemcpyDeviceToDevice;
  HIP_TRY(hipMemcpy(dst, src, bytes, k));
  return FMCW_OK;
}

int fmcw_device_count(int* n) {
  if (!n) return fail(FMCW_EINVAL, "null");
  *n = 0;
  if (hipGetDeviceCount(n) != hipSuccess) {
    (void)hipGetLastError();
    *n = 0;
  }
  return FMCW_OK;
}

}  // extern "C"
