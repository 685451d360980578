// fmcw_excise.hip -- the interference exciser of include/fmcw.h: an ADC cube in, the repaired cube, the
// per-sample mask, the per-chirp counts and four status words out.
//
// One memset of the status words and one launch per call (excise_kernel.hpp): persistent workgroups
// stride over the chirps, each chirp read once and written at most once.  The object owns no device
// memory.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "excise_kernel.hpp"
#include "internal.hpp"

using fmcw::fail;

static_assert(sizeof(fmcw_excise_config) == 48, "fmcw.h interference exciser layout");

namespace {

int validate(const fmcw_excise_config& c) {
  if (!fmcw::pow2(c.n_range) || c.n_range < 64 || c.n_range > 8192)
    return fail(FMCW_EINVAL, "n_range=%u: must be a power of two in [64, 8192]", c.n_range);
  if (c.n_doppler < 1 || c.n_doppler > 1024) return fail(FMCW_EINVAL, "n_doppler=%u: must be in [1, 1024]", c.n_doppler);
  if (c.n_rx < 1 || c.n_rx > 64) return fail(FMCW_EINVAL, "n_rx=%u: must be in [1, 64]", c.n_rx);
  if (c.in_dtype != FMCW_IN_F32 && c.in_dtype != FMCW_IN_F16 && c.in_dtype != FMCW_IN_I16)
    return fail(FMCW_EINVAL, "in_dtype %d (0 F32, 1 F16, 2 I16)", c.in_dtype);
  if (c.mode != FMCW_EXCISE_ZERO && c.mode != FMCW_EXCISE_INTERP)
    return fail(FMCW_EINVAL, "mode %d (0 ZERO, 1 INTERP)", c.mode);
  if (c.guard > 32) return fail(FMCW_EINVAL, "guard %u (0..32)", c.guard);
  if (c.rank_pct < 1 || c.rank_pct > 99) return fail(FMCW_EINVAL, "rank_pct %u (1..99)", c.rank_pct);
  if (!std::isfinite(c.alpha) || !(c.alpha >= 1.f)) return fail(FMCW_EINVAL, "alpha %g: must be finite and >= 1", c.alpha);
  if (c.max_frames < 1 || (uint64_t)c.max_frames * c.n_rx * c.n_doppler * c.n_range >= (1ull << 32))
    return fail(FMCW_EINVAL, "max_frames %u: need 1 <= max_frames and max_frames x samples < 2^32", c.max_frames);
  if (int rc = fmcw::check_device_id(c.device_id)) return rc;
  if (c.reserved[0] != 0 || c.reserved[1] != 0)
    return fail(FMCW_EINVAL, "reserved {%u, %u}: must be 0", c.reserved[0], c.reserved[1]);
  return FMCW_OK;
}

using ExFn = void (*)(const uint4*, uint4*, fmcw::ExciseArgs, uint32_t*, uint32_t*, uint32_t*);

// the instantiation for `vectors` 16-byte vectors per line: max(1, vectors / 256) per thread
template <class L>
ExFn pick(uint32_t vectors) {
  switch (std::max(1u, vectors / fmcw::kExNT)) {
    case 1: return fmcw::k_excise<L, 1>;
    case 2: return fmcw::k_excise<L, 2>;
    case 4: return fmcw::k_excise<L, 4>;
    case 8: return fmcw::k_excise<L, 8>;
    case 16: return L::V == 2 ? fmcw::k_excise<fmcw::ExF32, 16> : nullptr;   // 8192 complex64 only
  }
  return nullptr;
}

}  // namespace

struct fmcw_exciser {
  fmcw_excise_config cfg;
  ExFn fn = nullptr;
  fmcw::ExciseArgs args;
  size_t sample_bytes = 8;   // of one complex sample of the cube
  uint32_t max_grid = 1;     // workgroups resident at once (occupancy x CUs): the built-in bound
  uint32_t grid = 1;         // workgroups at most (fmcw_excise_set_grid_for_test)
};

extern "C" {

void fmcw_excise_config_default(fmcw_excise_config* cfg) {
  if (!cfg) return;
  cfg->n_range = 1024;
  cfg->n_doppler = 128;
  cfg->n_rx = 1;
  cfg->in_dtype = FMCW_IN_F32;
  cfg->mode = FMCW_EXCISE_ZERO;
  cfg->guard = 4;
  cfg->rank_pct = 50;
  cfg->alpha = 16.0f;
  cfg->max_frames = 1;
  cfg->device_id = 0;
  cfg->reserved[0] = cfg->reserved[1] = 0;
}

int fmcw_excise_create(const fmcw_excise_config* cfg, fmcw_exciser** out) {
  if (!cfg || !out) return fail(FMCW_EINVAL, "null argument");
  *out = nullptr;
  int rc = validate(*cfg);
  if (rc) return rc;
  hipDeviceProp_t prop;
  if ((rc = fmcw::open_device(cfg->device_id, &prop))) return rc;

  fmcw_exciser* e = new fmcw_exciser();
  e->cfg = *cfg;
  e->sample_bytes = cfg->in_dtype == FMCW_IN_F32 ? 8 : 4;
  const uint32_t vectors = (uint32_t)(cfg->n_range * e->sample_bytes / 16);
  e->fn = cfg->in_dtype == FMCW_IN_F32   ? pick<fmcw::ExF32>(vectors)
          : cfg->in_dtype == FMCW_IN_F16 ? pick<fmcw::ExF16>(vectors)
                                         : pick<fmcw::ExI16>(vectors);
  if (!e->fn) {
    delete e;
    return fail(FMCW_EINVAL, "n_range=%u: no k_excise instantiation", cfg->n_range);
  }
  fmcw::ExciseArgs& a = e->args;
  a.ns = cfg->n_range;
  a.n_lines = 0;
  a.k = (uint32_t)((uint64_t)cfg->n_range * cfg->rank_pct / 100);
  a.guard = cfg->guard;
  a.mode = cfg->mode;
  a.alpha = cfg->alpha;
  a.in_place = 0;
  e->max_grid = e->grid = fmcw::resident_grid(reinterpret_cast<const void*>(e->fn), fmcw::kExNT, 0, prop);
  *out = e;
  return FMCW_OK;
}

int fmcw_excise_destroy(fmcw_exciser* e) {
  delete e;
  return FMCW_OK;
}

int fmcw_excise_set_grid_for_test(fmcw_exciser* e, uint32_t grid) {
  if (!e) return fail(FMCW_EINVAL, "null exciser");
  e->grid = fmcw::clamp_grid(grid, e->max_grid);
  return FMCW_OK;
}

int fmcw_excise_enqueue(fmcw_exciser* e, const void* cube_dev, size_t n_frames, void* out_dev, uint32_t* mask_dev,
                        uint32_t* counts_dev, uint32_t* status_dev, void* stream) {
  if (!e) return fail(FMCW_EINVAL, "null exciser");
  if (!status_dev) return fail(FMCW_EINVAL, "null status_dev");
  if (!cube_dev) return fail(FMCW_EINVAL, "null cube_dev");
  if (!out_dev) return fail(FMCW_EINVAL, "null out_dev");
  if (n_frames < 1 || n_frames > e->cfg.max_frames)
    return fail(FMCW_EINVAL, "n_frames %zu: must be in 1..max_frames %u", n_frames, e->cfg.max_frames);
  if (int rc = fmcw::aligned(cube_dev, 16, "cube_dev")) return rc;
  if (int rc = fmcw::aligned(out_dev, 16, "out_dev")) return rc;
  if (int rc = fmcw::aligned(mask_dev, 4, "mask_dev")) return rc;
  if (int rc = fmcw::aligned(counts_dev, 4, "counts_dev")) return rc;
  if (int rc = fmcw::aligned(status_dev, 4, "status_dev")) return rc;
  const size_t lines = n_frames * e->cfg.n_rx * e->cfg.n_doppler;
  const size_t bytes = lines * e->cfg.n_range * e->sample_bytes;
  const uintptr_t src = reinterpret_cast<uintptr_t>(cube_dev), dst = reinterpret_cast<uintptr_t>(out_dev);
  if (src != dst && src < dst + bytes && dst < src + bytes)
    return fail(FMCW_EINVAL, "out_dev overlaps cube_dev: it must equal cube_dev (in place) or be disjoint");
  if (hipSetDevice(e->cfg.device_id) != hipSuccess) return fail(FMCW_EHIP, "hipSetDevice");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  HIP_TRY(hipMemsetAsync(status_dev, 0, 4 * sizeof(uint32_t), s));
  fmcw::ExciseArgs a = e->args;
  a.n_lines = (uint32_t)lines;   // max_frames x samples < 2^32
  a.in_place = src == dst;
  const uint32_t n_wg = (uint32_t)std::min<size_t>(lines, e->grid);
  hipLaunchKernelGGL(e->fn, dim3(n_wg), dim3(fmcw::kExNT), 0, s, static_cast<const uint4*>(cube_dev),
                     static_cast<uint4*>(out_dev), a, mask_dev, counts_dev, status_dev);
  return fmcw::check_launch("k_excise");
}

}  // extern "C"
