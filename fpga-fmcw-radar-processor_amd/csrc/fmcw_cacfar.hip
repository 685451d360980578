// fmcw_cacfar.hip -- the cell-averaging CFAR of include/fmcw.h (CA / GO / SO): a range-Doppler map
// in, the ordered fmcw_det list and its status words out.
//
// The reference's detectors are ordered-statistic; this is the detector whose cost does not depend on
// the data.  Three launches per call (cacfar_kernel.hpp): k_cacfar<false, *> counts per tile,
// k_cacfar_scan turns the counts into offsets and writes the status words, k_cacfar<true, *> recomputes
// and stores.  No atomic, no per-cell scratch: 8 B per tile.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "cacfar_kernel.hpp"
#include "internal.hpp"

using fmcw::fail;

static_assert(sizeof(fmcw_cacfar_config) == 48, "fmcw.h cell-averaging detector layout");

namespace {

// the largest any configuration needs (n_doppler 1024, window 8/4): 144 KiB of the CU's 160
constexpr size_t kMaxLdsBytes = (size_t)(25 + 9 + 2) * 1024 * sizeof(float);

// N of the window, in 64 bits (the fields are unchecked when it is first needed)
uint64_t n_ref(const fmcw_cacfar_config& c) {
  const uint64_t hr = (uint64_t)c.ref_range + c.guard_range, hd = (uint64_t)c.ref_doppler + c.guard_doppler;
  return (2 * hr + 1) * (2 * hd + 1) - (2 * (uint64_t)c.guard_range + 1) * (2 * (uint64_t)c.guard_doppler + 1);
}

int validate(const fmcw_cacfar_config& c) {
  if (int rc = fmcw::check_map_dims(c.n_range, c.n_doppler)) return rc;
  if (c.mode != FMCW_CACFAR_CA && c.mode != FMCW_CACFAR_GO && c.mode != FMCW_CACFAR_SO)
    return fail(FMCW_EINVAL, "mode %d (0 CA, 1 GO, 2 SO)", c.mode);
  if (c.ref_range > 8) return fail(FMCW_EINVAL, "ref_range %u (0..8)", c.ref_range);
  if (c.guard_range > 4) return fail(FMCW_EINVAL, "guard_range %u (0..4)", c.guard_range);
  if (c.ref_doppler > 8) return fail(FMCW_EINVAL, "ref_doppler %u (0..8)", c.ref_doppler);
  if (c.guard_doppler > 4) return fail(FMCW_EINVAL, "guard_doppler %u (0..4)", c.guard_doppler);
  if (n_ref(c) < 2)
    return fail(FMCW_EINVAL, "ref_range %u and ref_doppler %u: the window has no reference cell", c.ref_range,
                c.ref_doppler);
  if (2 * (c.ref_doppler + c.guard_doppler) + 1 > c.n_doppler)
    return fail(FMCW_EINVAL, "ref_doppler %u + guard_doppler %u: the window is wider than n_doppler %u", c.ref_doppler,
                c.guard_doppler, c.n_doppler);
  if (2 * (c.ref_range + c.guard_range) + 1 > c.n_range)
    return fail(FMCW_EINVAL, "ref_range %u + guard_range %u: the window is taller than n_range %u", c.ref_range,
                c.guard_range, c.n_range);
  if (!std::isfinite(c.alpha) || !(c.alpha > 0.f)) return fail(FMCW_EINVAL, "alpha %g: must be finite and > 0", c.alpha);
  if (c.max_frames < 1 || (uint64_t)c.max_frames * c.n_range * c.n_doppler >= (1ull << 32))
    return fail(FMCW_EINVAL, "max_frames %u: need 1 <= max_frames and max_frames x cells < 2^32", c.max_frames);
  if (int rc = fmcw::check_device_id(c.device_id)) return rc;
  if (c.reserved[0] != 0 || c.reserved[1] != 0)
    return fail(FMCW_EINVAL, "reserved {%u, %u}: must be 0", c.reserved[0], c.reserved[1]);
  return FMCW_OK;
}

}  // namespace

using CaFn = void (*)(const float*, fmcw::CaCfarArgs, int, uint32_t*, const uint32_t*, fmcw_det*, uint32_t);

struct fmcw_cacfar {
  fmcw_cacfar_config cfg;
  CaFn count = nullptr, emit = nullptr;   // the default window's instantiations, or the general ones
  fmcw::CaCfarArgs args;
  size_t lds_bytes = 0;        // dynamic LDS of a k_cacfar workgroup
  uint32_t max_grid = 1;       // workgroups resident at once (occupancy x CUs): the built-in bound
  uint32_t grid = 1;           // workgroups of the two passes at most (fmcw_cacfar_set_grid_for_test)
  uint32_t* tile_words = nullptr;  // counts[max_tiles], offs[max_tiles]
  size_t max_tiles = 0;
};

extern "C" {

void fmcw_cacfar_config_default(fmcw_cacfar_config* cfg) {
  if (!cfg) return;
  cfg->n_range = 1024;
  cfg->n_doppler = 128;
  cfg->mode = FMCW_CACFAR_CA;
  cfg->ref_range = 4;
  cfg->guard_range = 1;
  cfg->ref_doppler = 4;
  cfg->guard_doppler = 2;
  cfg->alpha = 4.0f;
  cfg->max_frames = 1;
  cfg->device_id = 0;
  cfg->reserved[0] = cfg->reserved[1] = 0;
}

int fmcw_cacfar_create(const fmcw_cacfar_config* cfg, fmcw_cacfar** out) {
  if (!cfg || !out) return fail(FMCW_EINVAL, "null argument");
  *out = nullptr;
  int rc = validate(*cfg);
  if (rc) return rc;
  hipDeviceProp_t prop;
  if ((rc = fmcw::open_device(cfg->device_id, &prop))) return rc;

  fmcw_cacfar* c = new fmcw_cacfar();
  c->cfg = *cfg;
  fmcw::CaCfarArgs& a = c->args;
  const int nd = (int)cfg->n_doppler, ns = (int)cfg->n_range;
  a.ns = ns;
  a.lg_nd = __builtin_ctz(cfg->n_doppler);
  a.mode = cfg->mode;
  a.rr = (int)cfg->ref_range;
  a.gr = (int)cfg->guard_range;
  a.rd = (int)cfg->ref_doppler;
  a.gd = (int)cfg->guard_doppler;
  const uint64_t n = n_ref(*cfg);
  a.k = cfg->mode == FMCW_CACFAR_CA ? (float)((double)cfg->alpha / (double)n) : (float)((double)cfg->alpha / (double)(n / 2));
  a.rps = std::max(1, fmcw::kCaStepCells / nd);
  a.strip = std::min(std::max(65536 / nd, 64), ns);
  a.tiles_per_frame = ns / a.strip;
  c->max_tiles = (size_t)cfg->max_frames * (size_t)a.tiles_per_frame;
  c->lds_bytes = fmcw::cacfar_lds_floats(nd, a.rr + a.gr, a.gr, a.rps) * sizeof(float);
  const bool def = a.rr == 4 && a.gr == 1 && a.rd == 4 && a.gd == 2;
  c->count = def ? fmcw::k_cacfar<false, true> : fmcw::k_cacfar<false, false>;
  c->emit = def ? fmcw::k_cacfar<true, true> : fmcw::k_cacfar<true, false>;
  const void* const count = reinterpret_cast<const void*>(c->count);
  const void* const emit = reinterpret_cast<const void*>(c->emit);
  if ((rc = fmcw::raise_lds_limit({count, emit}, kMaxLdsBytes, "k_cacfar"))) {
    delete c;
    return rc;
  }
  c->max_grid = c->grid = fmcw::resident_grid(emit, fmcw::kCaNT, c->lds_bytes, prop);
  if (!fmcw::alloc_scratch({fmcw::scratch(c->tile_words, 2 * c->max_tiles * sizeof(uint32_t))})) {
    const size_t tiles = c->max_tiles;
    delete c;
    return fail(FMCW_ENOMEM, "hipMalloc for the detector's %zu tile words failed", 2 * tiles);
  }
  *out = c;
  return FMCW_OK;
}

int fmcw_cacfar_destroy(fmcw_cacfar* c) {
  if (!c) return FMCW_OK;
  fmcw::free_scratch(c->cfg.device_id, {c->tile_words});
  delete c;
  return FMCW_OK;
}

int fmcw_cacfar_set_grid_for_test(fmcw_cacfar* c, uint32_t grid) {
  if (!c) return fail(FMCW_EINVAL, "null detector");
  c->grid = fmcw::clamp_grid(grid, c->max_grid);
  return FMCW_OK;
}

int fmcw_cacfar_enqueue(fmcw_cacfar* c, const float* map_dev, size_t n_frames, fmcw_det* dets_dev, size_t det_cap,
                        uint32_t* n_dets_dev, void* stream) {
  if (!c) return fail(FMCW_EINVAL, "null detector");
  if (!n_dets_dev) return fail(FMCW_EINVAL, "null n_dets_dev");
  if (n_frames > c->cfg.max_frames)
    return fail(FMCW_EINVAL, "n_frames %zu exceeds max_frames %u", n_frames, c->cfg.max_frames);
  if (int rc = fmcw::check_map_and_dets(map_dev, n_frames, dets_dev, det_cap)) return rc;
  if (hipSetDevice(c->cfg.device_id) != hipSuccess) return fail(FMCW_EHIP, "hipSetDevice");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int n_tiles = (int)(n_frames * (size_t)c->args.tiles_per_frame);
  uint32_t* const counts = c->tile_words;
  uint32_t* const offs = c->tile_words + c->max_tiles;
  const uint32_t n_wg = std::min((uint32_t)n_tiles, c->grid);
  // every index fits 32 bits: max_frames x cells < 2^32
  const uint32_t cap = (uint32_t)std::min<size_t>(det_cap, 0xffffffffu);
  if (n_tiles) {
    hipLaunchKernelGGL(c->count, dim3(n_wg), dim3(fmcw::kCaNT), c->lds_bytes, s, map_dev, c->args, n_tiles,
                       counts, static_cast<const uint32_t*>(nullptr), static_cast<fmcw_det*>(nullptr), 0u);
    if (int rc = fmcw::check_launch("k_cacfar count")) return rc;
  }
  hipLaunchKernelGGL(fmcw::k_cacfar_scan, dim3(1), dim3(fmcw::kCaScanNT), 0, s, static_cast<const uint32_t*>(counts),
                     offs, n_tiles, n_dets_dev);
  if (int rc = fmcw::check_launch("k_cacfar_scan")) return rc;
  if (n_tiles && cap) {
    hipLaunchKernelGGL(c->emit, dim3(n_wg), dim3(fmcw::kCaNT), c->lds_bytes, s, map_dev, c->args, n_tiles,
                       static_cast<uint32_t*>(nullptr), static_cast<const uint32_t*>(offs), dets_dev, cap);
    if (int rc = fmcw::check_launch("k_cacfar emit")) return rc;
  }
  return FMCW_OK;
}

}  // extern "C"
