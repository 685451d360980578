// fmcw_adapt.hip -- adaptive beam weights of include/fmcw.h: the corner-turned spectrum of
// fmcw_range_ct in, the minimum-variance (MVDR) weight matrix for fmcw_beams_set_weights_dev out.
//
// The reference is a single-channel core and has no such stage.  The beamformer applies whatever
// matrix its caller computed; this object computes one from the data: the sample covariance of the
// channels over a training window (adapt_kernel.hpp's k_adapt_acc: a real Gram matrix on the f32
// matrix cores, one partial tile per unit, no atomics) and the diagonally loaded solve under a
// unit-gain constraint per look direction (k_adapt_fold and k_adapt_solve: the units' tiles summed
// in a fixed order and the solve in one workgroup, fp64).  Three launches per call; every scratch
// word a launch reads is written by the one before it in the same call.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "adapt_kernel.hpp"
#include "internal.hpp"

using fmcw::fail;

static_assert(sizeof(fmcw_adapt_config) == 40, "fmcw.h adaptive-weights layout");
static_assert(FMCW_ADAPT_INFO_WORDS == 8, "k_adapt_solve writes 8 status words");

namespace {

using AccFn = void (*)(const float2*, fmcw::AdaptGeom, float*);

int validate(const fmcw_adapt_config& c) {
  if (int rc = fmcw::check_map_dims(c.n_range, c.n_doppler)) return rc;
  if (int rc = fmcw::check_n_rx(c.n_rx, 16)) return rc;
  if (c.n_beams < 1 || c.n_beams > 64) return fail(FMCW_EINVAL, "n_beams=%u: must be in [1, 64]", c.n_beams);
  if (int rc = fmcw::check_mti_mode(c.mti_mode)) return rc;
  if (c.train_rows < 1 || c.train_rows > c.n_range)
    return fail(FMCW_EINVAL, "train_rows=%u: must be in [1, n_range = %u]", c.train_rows, c.n_range);
  if (c.train_r0 > c.n_range - c.train_rows)
    return fail(FMCW_EINVAL, "train_r0=%u: rows [%u, %u) leave the map of n_range = %u", c.train_r0, c.train_r0,
                c.train_r0 + c.train_rows, c.n_range);
  if (!std::isfinite(c.loading) || c.loading < 0.f)
    return fail(FMCW_EINVAL, "loading %g: must be finite and >= 0", (double)c.loading);
  if (c.reserved != 0) return fail(FMCW_EINVAL, "reserved %u: must be 0", c.reserved);
  if (int rc = fmcw::check_device_id(c.device_id)) return rc;
  return FMCW_OK;
}

}  // namespace

struct fmcw_adapt {
  fmcw_adapt_config cfg;
  AccFn acc = nullptr;
  uint32_t rows = 32;      // the accumulator tile: 16 real rows for n_rx <= 8, else 32
  uint32_t max_grid = 1;   // workgroups of k_adapt_acc that can hold every unit
  uint32_t grid = 1;       // workgroups at most (fmcw_adapt_set_grid_for_test)
  float2* a = nullptr;     // the constraint matrix [beam][rx]
  float* part = nullptr;   // kAdaptMaxUnits partial tiles of rows x rows floats
  double* part2 = nullptr; // kAdaptFoldParts tiles of rows x rows doubles
};

extern "C" {

void fmcw_adapt_config_default(fmcw_adapt_config* cfg) {
  if (!cfg) return;
  cfg->n_range = 1024;
  cfg->n_doppler = 128;
  cfg->n_rx = 1;
  cfg->n_beams = 1;
  cfg->mti_mode = FMCW_MTI_OFF;
  cfg->train_r0 = 0;
  cfg->train_rows = 1024;
  cfg->loading = 1e-2f;
  cfg->reserved = 0;
  cfg->device_id = 0;
}

int fmcw_adapt_create(const fmcw_adapt_config* cfg, const float* a_host, fmcw_adapt** out) {
  if (!cfg || !out) return fail(FMCW_EINVAL, "null argument");
  *out = nullptr;
  int rc = validate(*cfg);
  if (rc) return rc;
  if (!a_host) return fail(FMCW_EINVAL, "null a_host");
  for (uint32_t b = 0; b < cfg->n_beams; ++b) {
    bool any = false;
    for (uint32_t k = 0; k < cfg->n_rx; ++k)
      for (int h = 0; h < 2; ++h) {
        const float v = a_host[2 * ((size_t)b * cfg->n_rx + k) + h];
        if (!std::isfinite(v)) return fail(FMCW_EINVAL, "a_host: beam %u, rx %u is not finite", b, k);
        any = any || v != 0.f;
      }
    if (!any) return fail(FMCW_EINVAL, "a_host: beam %u is all zero (no look direction to hold at unit gain)", b);
  }
  if ((rc = fmcw::open_device(cfg->device_id))) return rc;
  fmcw_adapt* a = new fmcw_adapt();
  a->cfg = *cfg;
  a->rows = cfg->n_rx <= 8 ? 16 : 32;
  a->acc = fmcw::with_mti(cfg->mti_mode, [a](auto m) -> AccFn {
    constexpr int M = decltype(m)::value;
    return a->rows == 16 ? fmcw::k_adapt_acc<16, M> : fmcw::k_adapt_acc<32, M>;
  });
  a->max_grid = a->grid = fmcw::kAdaptMaxUnits / fmcw::kAdaptWaves;
  const size_t na = (size_t)cfg->n_beams * cfg->n_rx;
  const size_t n_part = (size_t)fmcw::kAdaptMaxUnits * a->rows * a->rows;
  const size_t part2_bytes = (size_t)fmcw::kAdaptFoldParts * a->rows * a->rows * sizeof(double);
  if (!fmcw::alloc_scratch({fmcw::scratch(a->a, na * sizeof(float2)), fmcw::scratch(a->part, n_part * sizeof(float)),
                            fmcw::scratch(a->part2, part2_bytes)})) {
    fmcw_adapt_destroy(a);
    return fail(FMCW_ENOMEM, "hipMalloc for the constraint matrix (%zu) and the partial tiles (%zu floats) failed", na,
                n_part);
  }
  if (!fmcw::upload_tables({{a->a, a_host, na * sizeof(float2)}})) {
    fmcw_adapt_destroy(a);
    return fail(FMCW_EHIP, "upload of the constraint matrix failed");
  }
  *out = a;
  return FMCW_OK;
}

int fmcw_adapt_destroy(fmcw_adapt* a) {
  if (!a) return FMCW_OK;
  fmcw::free_scratch(a->cfg.device_id, {a->a, a->part, a->part2});
  delete a;
  return FMCW_OK;
}

int fmcw_adapt_set_grid_for_test(fmcw_adapt* a, uint32_t grid) {
  if (!a) return fail(FMCW_EINVAL, "null adaptive-weights object");
  a->grid = fmcw::clamp_grid(grid, a->max_grid);
  return FMCW_OK;
}

int fmcw_adapt_enqueue(fmcw_adapt* a, const void* spec_dev, size_t n_frames, void* w_dev, void* cov_dev,
                       uint32_t* info_dev, void* stream) {
  if (!a) return fail(FMCW_EINVAL, "null adaptive-weights object");
  if (n_frames == 0) return FMCW_OK;
  if (!spec_dev || !w_dev || !info_dev)
    return fail(FMCW_EINVAL, "null spec_dev, w_dev or info_dev with n_frames %zu", n_frames);
  if (int rc = fmcw::aligned(spec_dev, 8, "spec_dev")) return rc;
  if (int rc = fmcw::aligned(w_dev, 8, "w_dev")) return rc;
  if (int rc = fmcw::aligned(cov_dev, 16, "cov_dev")) return rc;
  if (int rc = fmcw::aligned(info_dev, 4, "info_dev")) return rc;
  const fmcw_adapt_config& c = a->cfg;
  fmcw::AdaptGeom g;
  g.nd = c.n_doppler;
  g.nrx = c.n_rx;
  g.cf = c.train_rows * c.n_doppler;
  g.spf = (g.cf + 63u) / 64u;
  if (n_frames > 0x7fffffffu / g.spf)
    return fail(FMCW_EINVAL, "n_frames %zu: more than 2^31 - 1 steps of 64 training cells (%u per frame)", n_frames,
                g.spf);
  g.n_steps = (uint32_t)n_frames * g.spf;
  g.n_units = std::min(g.n_steps, (uint32_t)fmcw::kAdaptMaxUnits);
  g.off0 = c.train_r0 * c.n_doppler;
  g.rx_step = c.n_range * c.n_doppler;
  if (hipSetDevice(c.device_id) != hipSuccess) return fail(FMCW_EHIP, "hipSetDevice");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const uint32_t n_wg = std::min((g.n_units + fmcw::kAdaptWaves - 1) / fmcw::kAdaptWaves, a->grid);
  hipLaunchKernelGGL(a->acc, dim3(n_wg), dim3(fmcw::kAdaptThreads), 0, s, static_cast<const float2*>(spec_dev), g,
                     a->part);
  if (int rc = fmcw::check_launch("k_adapt_acc")) return rc;
  const uint32_t n_parts = std::min(g.n_units, (uint32_t)fmcw::kAdaptFoldParts);
  hipLaunchKernelGGL(fmcw::k_adapt_fold, dim3(n_parts), dim3(256), 0, s, static_cast<const float*>(a->part), g.n_units,
                     n_parts, a->rows * a->rows, a->part2);
  if (int rc = fmcw::check_launch("k_adapt_fold")) return rc;
  fmcw::SolveArgs p;
  p.nrx = c.n_rx;
  p.nb = c.n_beams;
  p.rows = a->rows;
  p.n_units = g.n_units;
  p.n_parts = n_parts;
  p.K = (uint64_t)n_frames * g.cf;
  p.loading = (double)c.loading;
  hipLaunchKernelGGL(fmcw::k_adapt_solve, dim3(1), dim3(fmcw::kSolveThreads), 0, s,
                     static_cast<const double*>(a->part2), static_cast<const float2*>(a->a), p,
                     static_cast<float2*>(w_dev), static_cast<double2*>(cov_dev), info_dev);
  return fmcw::check_launch("k_adapt_solve");
}

}  // extern "C"
