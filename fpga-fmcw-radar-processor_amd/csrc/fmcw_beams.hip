// fmcw_beams.hip -- coherent beamforming of include/fmcw.h: the corner-turned spectrum of
// fmcw_range_ct in, one range-Doppler magnitude map per (frame, beam) out, ready for fmcw_cfar.
//
// The reference is a single-channel core and has no such stage.  With n_rx > 1 the Doppler stage
// sums the channels' powers (NCI); here a caller-supplied complex matrix W [beam][rx] is applied to
// the channels before the Doppler transform, so a beam steered at a target gains n_rx in SNR
// instead of sqrt(n_rx).  The kernel is beam_kernel.hpp's k_beams, K2's sibling: the same wave
// tiles, FFT passes and map store, one persistent launch per call, no scratch and no counter.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "beam_kernel.hpp"
#include "internal.hpp"

using fmcw::fail;

static_assert(sizeof(fmcw_beams_config) == 32, "fmcw.h beamformer layout");

namespace {

using BeamFn = void (*)(const float2*, const float2*, const float*, int, int, int, int, float*);

struct BeamKernel {
  BeamFn fn;
  int WR, NT;  // range rows per wave tile, threads per workgroup
};

template <int NC>
BeamKernel pick_mti(int mti) {
  using Gm = fmcw::DopplerGeom<NC>;
  return {fmcw::with_mti(mti, [](auto m) -> BeamFn { return fmcw::k_beams<NC, decltype(m)::value>; }), Gm::WR, Gm::NT};
}

BeamKernel pick(uint32_t nd, int mti) {
  switch (nd) {
    case 32: return pick_mti<32>(mti);
    case 64: return pick_mti<64>(mti);
    case 128: return pick_mti<128>(mti);
    case 256: return pick_mti<256>(mti);
    case 512: return pick_mti<512>(mti);
    default: return pick_mti<1024>(mti);
  }
}

int validate(const fmcw_beams_config& c) {
  if (int rc = fmcw::check_map_dims(c.n_range, c.n_doppler)) return rc;
  if (int rc = fmcw::check_n_rx(c.n_rx, 64)) return rc;
  if (c.n_beams < 1 || c.n_beams > 64) return fail(FMCW_EINVAL, "n_beams=%u: must be in [1, 64]", c.n_beams);
  if (int rc = fmcw::check_float_window(c.window, "beamformer")) return rc;
  if (int rc = fmcw::check_mti_mode(c.mti_mode)) return rc;
  if (c.reserved != 0) return fail(FMCW_EINVAL, "reserved %u: must be 0", c.reserved);
  if (int rc = fmcw::check_device_id(c.device_id)) return rc;
  return FMCW_OK;
}

}  // namespace

struct fmcw_beams {
  fmcw_beams_config cfg;
  BeamKernel k;
  uint32_t max_grid = 1;   // workgroups resident at once (occupancy x CUs): the built-in bound
  uint32_t grid = 1;       // workgroups of k_beams at most (fmcw_beams_set_grid_for_test)
  float2* w = nullptr;     // the weight matrix [beam][rx]
  float* win = nullptr;    // the Doppler window, n_doppler
};

extern "C" {

void fmcw_beams_config_default(fmcw_beams_config* cfg) {
  if (!cfg) return;
  cfg->n_range = 1024;
  cfg->n_doppler = 128;
  cfg->n_rx = 1;
  cfg->n_beams = 1;
  cfg->window = FMCW_WIN_HAMMING;
  cfg->mti_mode = FMCW_MTI_OFF;
  cfg->reserved = 0;
  cfg->device_id = 0;
}

int fmcw_beams_create(const fmcw_beams_config* cfg, const float* weights_host, fmcw_beams** out) {
  if (!cfg || !out) return fail(FMCW_EINVAL, "null argument");
  *out = nullptr;
  int rc = validate(*cfg);
  if (rc) return rc;
  if (!weights_host) return fail(FMCW_EINVAL, "null weights_host");
  const size_t nw = (size_t)cfg->n_beams * cfg->n_rx;
  for (size_t i = 0; i < 2 * nw; ++i)
    if (!std::isfinite(weights_host[i]))
      return fail(FMCW_EINVAL, "weights_host: beam %zu, rx %zu is not finite", i / 2 / cfg->n_rx, i / 2 % cfg->n_rx);
  hipDeviceProp_t prop;
  if ((rc = fmcw::open_device(cfg->device_id, &prop))) return rc;
  const uint32_t nd = cfg->n_doppler;
  const std::vector<float> win = fmcw::window_table(nd, cfg->window);
  fmcw_beams* b = new fmcw_beams();
  b->cfg = *cfg;
  b->k = pick(nd, cfg->mti_mode);
  b->max_grid = b->grid = fmcw::resident_grid(reinterpret_cast<const void*>(b->k.fn), b->k.NT, 0, prop);
  if (!fmcw::alloc_scratch({fmcw::scratch(b->w, nw * sizeof(float2)), fmcw::scratch(b->win, nd * sizeof(float))})) {
    fmcw_beams_destroy(b);
    return fail(FMCW_ENOMEM, "hipMalloc for the beamformer's weights (%zu) and window (%u entries) failed", nw, nd);
  }
  if (!fmcw::upload_tables({{b->w, weights_host, nw * sizeof(float2)}, {b->win, win.data(), nd * sizeof(float)}})) {
    fmcw_beams_destroy(b);
    return fail(FMCW_EHIP, "upload of the beamformer's weights and window failed");
  }
  *out = b;
  return FMCW_OK;
}

int fmcw_beams_destroy(fmcw_beams* b) {
  if (!b) return FMCW_OK;
  fmcw::free_scratch(b->cfg.device_id, {b->w, b->win});
  delete b;
  return FMCW_OK;
}

int fmcw_beams_set_grid_for_test(fmcw_beams* b, uint32_t grid) {
  if (!b) return fail(FMCW_EINVAL, "null beamformer");
  b->grid = fmcw::clamp_grid(grid, b->max_grid);
  return FMCW_OK;
}

int fmcw_beams_set_weights_dev(fmcw_beams* b, const void* w_dev, void* stream) {
  if (!b) return fail(FMCW_EINVAL, "null beamformer");
  if (!w_dev) return fail(FMCW_EINVAL, "null w_dev");
  if (int rc = fmcw::aligned(w_dev, 8, "w_dev")) return rc;
  if (hipSetDevice(b->cfg.device_id) != hipSuccess) return fail(FMCW_EHIP, "hipSetDevice");
  HIP_TRY(hipMemcpyAsync(b->w, w_dev, (size_t)b->cfg.n_beams * b->cfg.n_rx * sizeof(float2), hipMemcpyDeviceToDevice,
                         reinterpret_cast<hipStream_t>(stream)));
  return FMCW_OK;
}

int fmcw_beams_enqueue(fmcw_beams* b, const void* spec_dev, size_t n_frames, float* maps_dev, void* stream) {
  if (!b) return fail(FMCW_EINVAL, "null beamformer");
  if (n_frames == 0) return FMCW_OK;
  if (!spec_dev || !maps_dev) return fail(FMCW_EINVAL, "null spec_dev or maps_dev with n_frames %zu", n_frames);
  if (int rc = fmcw::aligned(maps_dev, 16, "maps_dev")) return rc;
  if (int rc = fmcw::aligned(spec_dev, 8, "spec_dev")) return rc;
  const fmcw_beams_config& c = b->cfg;
  const size_t tiles_frame = c.n_range / (uint32_t)b->k.WR;
  if (n_frames > 0x7fffffffu / tiles_frame)
    return fail(FMCW_EINVAL, "n_frames %zu: more than 2^31 - 1 wave tiles (%zu per frame)", n_frames, tiles_frame);
  if (hipSetDevice(c.device_id) != hipSuccess) return fail(FMCW_EHIP, "hipSetDevice");
  const int n_tiles = (int)(n_frames * tiles_frame);
  const int wpb = b->k.NT / 64;
  const uint32_t n_wg = std::min((uint32_t)(((int64_t)n_tiles + wpb - 1) / wpb), b->grid);
  hipLaunchKernelGGL(b->k.fn, dim3(n_wg), dim3(b->k.NT), 0, reinterpret_cast<hipStream_t>(stream),
                     static_cast<const float2*>(spec_dev), static_cast<const float2*>(b->w),
                     static_cast<const float*>(b->win), (int)c.n_range, (int)c.n_rx, (int)c.n_beams, n_tiles, maps_dev);
  return fmcw::check_launch("k_beams");
}

}  // extern "C"
