// fmcw_doa.hip -- the angle resolver of include/fmcw.h: the channel snapshots of fmcw_bearings_enqueue
// and a caller-supplied steering table in, up to four sources per record (grid point, refined position,
// complex amplitude) out.  The kernels and their design are doa_kernel.hpp's: k_doa_table when the table
// is set, then per call k_doa and k_bearings_status.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "doa_kernel.hpp"
#include "internal.hpp"

using fmcw::fail;

static_assert(sizeof(fmcw_doa) == 96 && sizeof(fmcw_doa_src) == 16 && sizeof(fmcw_doa_config) == 32, "fmcw.h angle resolver layouts");

namespace {

using fmcw::kDoaMaxGrid;
using DoaFn = decltype(&fmcw::k_doa<1>);

// the instantiation with the fewest register slots per lane that hold n_grid / 64 grid points
DoaFn pick(uint32_t n_grid) {
  const uint32_t m = n_grid / 64;
  if (m <= 1) return fmcw::k_doa<1>;
  if (m <= 2) return fmcw::k_doa<2>;
  if (m <= 4) return fmcw::k_doa<4>;
  if (m <= 8) return fmcw::k_doa<8>;
  return fmcw::k_doa<16>;
}

int validate(const fmcw_doa_config& c) {
  if (c.n_ch < 1 || c.n_ch > 64) return fail(FMCW_EINVAL, "n_ch=%u: must be in [1, 64]", c.n_ch);
  if (c.n_grid < 64 || c.n_grid > 1024 || c.n_grid % 64)
    return fail(FMCW_EINVAL, "n_grid=%u: must be a multiple of 64 in [64, 1024]", c.n_grid);
  if (c.k_max < 1 || c.k_max > FMCW_DOA_MAX_SRC) return fail(FMCW_EINVAL, "k_max=%u: must be in [1, 4]", c.k_max);
  if (c.relax_passes > 3) return fail(FMCW_EINVAL, "relax_passes=%u: must be in [0, 3]", c.relax_passes);
  if (!(c.min_rel >= 0.f && c.min_rel < 1.f)) return fail(FMCW_EINVAL, "min_rel %g: must be in [0, 1)", (double)c.min_rel);
  if (c.refine > 1) return fail(FMCW_EINVAL, "refine=%u: must be 0 or 1", c.refine);
  if (c.max_records < 1 || c.max_records > 0x7fffffffu)
    return fail(FMCW_EINVAL, "max_records %u (1..2^31-1)", c.max_records);
  if (int rc = fmcw::check_device_id(c.device_id)) return rc;
  return FMCW_OK;
}

}  // namespace

struct fmcw_doa_resolver {
  fmcw_doa_config cfg;
  DoaFn kern = nullptr;           // k_doa of this n_grid
  uint32_t grid = kDoaMaxGrid;    // workgroups of it at most (fmcw_doa_set_grid_for_test)
  float2* a_in = nullptr;         // A[g][k] as fmcw_doa_set_steering uploads it
  float2* at = nullptr;           // At[k][g], what k_doa reads
  float* w = nullptr;             // w[g]
  uint32_t* wg_bad = nullptr;     // kDoaMaxGrid words: records without a snapshot per workgroup of the call
  size_t table_bytes() const { return (size_t)cfg.n_grid * cfg.n_ch * sizeof(float2); }
};

extern "C" {

void fmcw_doa_config_default(fmcw_doa_config* cfg) {
  if (!cfg) return;
  cfg->n_ch = 16;
  cfg->n_grid = 256;
  cfg->k_max = 2;
  cfg->relax_passes = 2;
  cfg->min_rel = 0.02f;
  cfg->refine = 1;
  cfg->max_records = 1u << 20;
  cfg->device_id = 0;
}

int fmcw_doa_create(const fmcw_doa_config* cfg, fmcw_doa_resolver** out) {
  if (!cfg || !out) return fail(FMCW_EINVAL, "null argument");
  *out = nullptr;
  int rc = validate(*cfg);
  if (rc) return rc;
  if ((rc = fmcw::open_device(cfg->device_id))) return rc;
  fmcw_doa_resolver* d = new fmcw_doa_resolver();
  d->cfg = *cfg;
  d->kern = pick(cfg->n_grid);
  const size_t wb = cfg->n_grid * sizeof(float);
  if (!fmcw::alloc_scratch({fmcw::scratch(d->a_in, d->table_bytes()), fmcw::scratch(d->at, d->table_bytes()),
                            fmcw::scratch(d->w, wb), fmcw::scratch(d->wg_bad, kDoaMaxGrid * sizeof(uint32_t))})) {
    fmcw_doa_destroy(d);
    return fail(FMCW_ENOMEM, "hipMalloc for the angle resolver's steering table (%u x %u) failed", cfg->n_grid, cfg->n_ch);
  }
  if (hipMemset(d->at, 0, d->table_bytes()) != hipSuccess || hipMemset(d->w, 0, wb) != hipSuccess) {
    (void)hipGetLastError();
    fmcw_doa_destroy(d);
    return fail(FMCW_EHIP, "clearing the angle resolver's steering table failed");
  }
  *out = d;
  return FMCW_OK;
}

int fmcw_doa_destroy(fmcw_doa_resolver* d) {
  if (!d) return FMCW_OK;
  fmcw::free_scratch(d->cfg.device_id, {d->a_in, d->at, d->w, d->wg_bad});
  delete d;
  return FMCW_OK;
}

int fmcw_doa_set_grid_for_test(fmcw_doa_resolver* d, uint32_t grid) {
  if (!d) return fail(FMCW_EINVAL, "null angle resolver");
  d->grid = fmcw::clamp_grid(grid, kDoaMaxGrid);
  return FMCW_OK;
}

int fmcw_doa_set_steering_dev(fmcw_doa_resolver* d, const void* steering_dev, void* stream) {
  if (!d) return fail(FMCW_EINVAL, "null angle resolver");
  if (!steering_dev) return fail(FMCW_EINVAL, "null steering_dev");
  if (int rc = fmcw::aligned(steering_dev, 8, "steering_dev")) return rc;
  if (hipSetDevice(d->cfg.device_id) != hipSuccess) return fail(FMCW_EHIP, "hipSetDevice");
  hipLaunchKernelGGL(fmcw::k_doa_table, dim3(d->cfg.n_grid / 64), dim3(64), 0, reinterpret_cast<hipStream_t>(stream),
                     static_cast<const float2*>(steering_dev), d->cfg.n_ch, d->cfg.n_grid, d->at, d->w);
  return fmcw::check_launch("k_doa_table");
}

int fmcw_doa_set_steering(fmcw_doa_resolver* d, const float* steering_host, void* stream) {
  if (!d) return fail(FMCW_EINVAL, "null angle resolver");
  if (!steering_host) return fail(FMCW_EINVAL, "null steering_host");
  const uint32_t nch = d->cfg.n_ch;
  for (uint32_t g = 0; g < d->cfg.n_grid; ++g) {   // k_doa_table's sum: squares of fp32 are exact in fp64
    double norm = 0.0;
    for (uint32_t k = 0; k < nch; ++k) {
      const double re = steering_host[2 * ((size_t)g * nch + k)], im = steering_host[2 * ((size_t)g * nch + k) + 1];
      norm += re * re + im * im;
    }
    if (!(norm > 0.0) || !std::isfinite(norm))
      return fail(FMCW_EINVAL, "steering_host: row %u has norm %g, must be positive and finite", g, norm);
  }
  if (hipSetDevice(d->cfg.device_id) != hipSuccess) return fail(FMCW_EHIP, "hipSetDevice");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  HIP_TRY(hipMemcpyAsync(d->a_in, steering_host, d->table_bytes(), hipMemcpyHostToDevice, s));
  if (int rc = fmcw_doa_set_steering_dev(d, d->a_in, stream)) return rc;
  HIP_TRY(hipStreamSynchronize(s));   // steering_host is the caller's again, and a_in free for the next table
  return FMCW_OK;
}

int fmcw_doa_enqueue(fmcw_doa_resolver* d, const void* snaps_dev, const void* cells_dev, size_t cell_stride,
                     size_t rec_cap, const uint32_t* n_records_dev, fmcw_doa* doa_dev, float* spectrum_dev,
                     uint32_t* n_out_dev, void* stream) {
  if (!d || !n_records_dev || !n_out_dev) return fail(FMCW_EINVAL, "null argument");
  if (cells_dev && cell_stride != 16 && cell_stride != 32)
    return fail(FMCW_EINVAL, "cell_stride %zu (16 or 32)", cell_stride);
  if (rec_cap && (!snaps_dev || !doa_dev)) return fail(FMCW_EINVAL, "null snaps_dev or doa_dev with rec_cap %zu", rec_cap);
  if (int rc = fmcw::aligned(snaps_dev, 8, "snaps_dev")) return rc;
  if (int rc = fmcw::aligned(cells_dev, 4, "cells_dev")) return rc;
  if (int rc = fmcw::aligned(doa_dev, 16, "doa_dev")) return rc;
  if (int rc = fmcw::aligned(spectrum_dev, 4, "spectrum_dev")) return rc;
  if (hipSetDevice(d->cfg.device_id) != hipSuccess) return fail(FMCW_EHIP, "hipSetDevice");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const fmcw_doa_config& c = d->cfg;
  const uint32_t cap = (uint32_t)std::min<size_t>(rec_cap, c.max_records);  // n = min(n_records_dev[0], cap)
  const uint32_t n_wg = std::min((uint32_t)(((uint64_t)cap + fmcw::kDoaWaves - 1) / fmcw::kDoaWaves), d->grid);
  const fmcw::DoaGeom g = {c.n_ch, c.n_grid, c.k_max, c.relax_passes, c.refine, c.min_rel};
  if (n_wg) {
    hipLaunchKernelGGL(d->kern, dim3(n_wg), dim3(fmcw::kDoaThreads), 0, s, static_cast<const float2*>(snaps_dev),
                       static_cast<const uint8_t*>(cells_dev), (uint32_t)cell_stride, cap, n_records_dev, g, d->at, d->w,
                       doa_dev, spectrum_dev, d->wg_bad);
    if (int rc = fmcw::check_launch("k_doa")) return rc;
  }
  hipLaunchKernelGGL(fmcw::k_bearings_status, dim3(1), dim3(64), 0, s, cap, n_records_dev, d->wg_bad, n_wg, n_out_dev);
  return fmcw::check_launch("k_bearings_status");
}

}  // extern "C"
