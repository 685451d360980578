// fmcw_bearings.hip -- bearing estimation of include/fmcw.h: a detection or plot list and the
// corner-turned spectrum of fmcw_range_ct in, one fmcw_bearing (and the rx snapshot) per record out.
// The kernels and their design are bearings_kernel.hpp's: k_bearings, then k_bearings_status.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "bearings_kernel.hpp"
#include "internal.hpp"

using fmcw::fail;

static_assert(sizeof(fmcw_bearing) == 32 && sizeof(fmcw_bearings_config) == 32, "fmcw.h bearing layouts");

namespace {

using fmcw::kBearMaxGrid;
using BearFn = decltype(&fmcw::k_bearings<FMCW_MTI_OFF>);

int validate(const fmcw_bearings_config& c) {
  if (int rc = fmcw::check_map_dims(c.n_range, c.n_doppler)) return rc;
  if (int rc = fmcw::check_n_rx(c.n_rx, 64)) return rc;
  if (int rc = fmcw::check_float_window(c.window, "bearing estimator")) return rc;
  if (int rc = fmcw::check_mti_mode(c.mti_mode)) return rc;
  if (!(c.spacing > 0.f) || !std::isfinite(c.spacing))
    return fail(FMCW_EINVAL, "spacing %g: must be positive and finite (wavelengths)", (double)c.spacing);
  if (c.max_records < 1 || c.max_records > 0x7fffffffu)
    return fail(FMCW_EINVAL, "max_records %u (1..2^31-1)", c.max_records);
  if (int rc = fmcw::check_device_id(c.device_id)) return rc;
  return FMCW_OK;
}

}  // namespace

struct fmcw_bearings {
  fmcw_bearings_config cfg;
  BearFn kern = nullptr;       // k_bearings of this mti_mode
  uint32_t grid = kBearMaxGrid;  // workgroups of it at most (fmcw_bearings_set_grid_for_test)
  float2* tw = nullptr;        // exp(-2 pi i m / n_doppler), m < n_doppler
  float* win = nullptr;        // the Doppler window, n_doppler
  uint32_t* wg_bad = nullptr;  // kBearMaxGrid words: out-of-range records per workgroup of the call
};

extern "C" {

void fmcw_bearings_config_default(fmcw_bearings_config* cfg) {
  if (!cfg) return;
  cfg->n_range = 1024;
  cfg->n_doppler = 128;
  cfg->n_rx = 1;
  cfg->window = FMCW_WIN_HAMMING;
  cfg->mti_mode = FMCW_MTI_OFF;
  cfg->spacing = 0.5f;
  cfg->max_records = 1u << 20;
  cfg->device_id = 0;
}

int fmcw_bearings_create(const fmcw_bearings_config* cfg, fmcw_bearings** out) {
  if (!cfg || !out) return fail(FMCW_EINVAL, "null argument");
  *out = nullptr;
  int rc = validate(*cfg);
  if (rc) return rc;
  if ((rc = fmcw::open_device(cfg->device_id))) return rc;
  const uint32_t nd = cfg->n_doppler;
  std::vector<float2> tw(nd);
  for (uint32_t m = 0; m < nd; ++m) {
    const double a = -2.0 * M_PI * (double)m / (double)nd;
    tw[m] = make_float2((float)std::cos(a), (float)std::sin(a));
  }
  const std::vector<float> win = fmcw::window_table(nd, cfg->window);
  fmcw_bearings* b = new fmcw_bearings();
  b->cfg = *cfg;
  b->kern = fmcw::with_mti(cfg->mti_mode, [](auto m) -> BearFn { return fmcw::k_bearings<decltype(m)::value>; });
  if (!fmcw::alloc_scratch({fmcw::scratch(b->tw, nd * sizeof(float2)), fmcw::scratch(b->win, nd * sizeof(float)),
                            fmcw::scratch(b->wg_bad, kBearMaxGrid * sizeof(uint32_t))})) {
    fmcw_bearings_destroy(b);
    return fail(FMCW_ENOMEM, "hipMalloc for the bearing estimator's tables (%u entries) failed", nd);
  }
  if (!fmcw::upload_tables({{b->tw, tw.data(), nd * sizeof(float2)}, {b->win, win.data(), nd * sizeof(float)}})) {
    fmcw_bearings_destroy(b);
    return fail(FMCW_EHIP, "upload of the bearing estimator's tables failed");
  }
  *out = b;
  return FMCW_OK;
}

int fmcw_bearings_destroy(fmcw_bearings* b) {
  if (!b) return FMCW_OK;
  fmcw::free_scratch(b->cfg.device_id, {b->tw, b->win, b->wg_bad});
  delete b;
  return FMCW_OK;
}

int fmcw_bearings_set_grid_for_test(fmcw_bearings* b, uint32_t grid) {
  if (!b) return fail(FMCW_EINVAL, "null bearing estimator");
  b->grid = fmcw::clamp_grid(grid, kBearMaxGrid);
  return FMCW_OK;
}

int fmcw_bearings_enqueue(fmcw_bearings* b, const void* spec_dev, size_t n_frames, const void* records_dev,
                          size_t rec_stride, size_t rec_cap, const uint32_t* n_records_dev,
                          fmcw_bearing* bearings_dev, void* snaps_dev, uint32_t* n_out_dev, void* stream) {
  if (!b || !n_records_dev || !n_out_dev) return fail(FMCW_EINVAL, "null argument");
  if (rec_stride != sizeof(fmcw_det) && rec_stride != sizeof(fmcw_plot))
    return fail(FMCW_EINVAL, "rec_stride %zu (16 = fmcw_det, 32 = fmcw_plot)", rec_stride);
  if (n_frames > 0xffffffffu) return fail(FMCW_EINVAL, "n_frames %zu (< 2^32)", n_frames);
  if (n_frames && !spec_dev) return fail(FMCW_EINVAL, "null spec_dev with n_frames %zu", n_frames);
  if (rec_cap && (!records_dev || !bearings_dev))
    return fail(FMCW_EINVAL, "null records_dev or bearings_dev with rec_cap %zu", rec_cap);
  if (hipSetDevice(b->cfg.device_id) != hipSuccess) return fail(FMCW_EHIP, "hipSetDevice");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const fmcw_bearings_config& c = b->cfg;
  const uint32_t cap = (uint32_t)std::min<size_t>(rec_cap, c.max_records);  // n = min(n_records_dev[0], cap)
  const uint32_t n_wg = std::min((uint32_t)(((uint64_t)cap + fmcw::kBearWaves - 1) / fmcw::kBearWaves), b->grid);
  const fmcw::BearGeom g = {(uint32_t)n_frames, c.n_range, c.n_doppler, c.n_rx, 1.0f / c.spacing};
  if (n_wg) {
    hipLaunchKernelGGL(b->kern, dim3(n_wg), dim3(fmcw::kBearThreads), 0, s, static_cast<const float2*>(spec_dev),
                       static_cast<const uint8_t*>(records_dev), (uint32_t)rec_stride, cap, n_records_dev, g, b->tw,
                       b->win, bearings_dev, static_cast<float2*>(snaps_dev), b->wg_bad);
    if (int rc = fmcw::check_launch("k_bearings")) return rc;
  }
  hipLaunchKernelGGL(fmcw::k_bearings_status, dim3(1), dim3(64), 0, s, cap, n_records_dev, b->wg_bad, n_wg, n_out_dev);
  return fmcw::check_launch("k_bearings_status");
}

}  // extern "C"
