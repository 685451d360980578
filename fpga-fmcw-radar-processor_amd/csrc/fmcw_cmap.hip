// fmcw_cmap.hip -- the clutter map of include/fmcw.h: range-Doppler maps in, the ordered fmcw_det list of
// the cells that exceed a multiple of their own history out, and that history kept on the device.
//
// Three launches per call whatever n_frames is (cmap_kernel.hpp): k_cmap<false, *> runs the call's scans
// per (stream, tile) unit and counts per (frame, tile) without touching the state, k_cmap_scan turns the
// counts into offsets, writes the status words and moves the ages and the current copy on, k_cmap<true, *>
// repeats the arithmetic, stores the records and writes the planes' other copy.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>

#include "cmap_kernel.hpp"
#include "internal.hpp"

using fmcw::fail;

static_assert(sizeof(fmcw_cmap_config) == 64, "fmcw.h clutter map layout");

namespace {

// the largest any configuration needs: n_doppler 1024 (8 owned rows), spread_range 4
constexpr size_t kMaxLdsBytes = (size_t)(8 + 2 * fmcw::kCmMaxSpread) * 1024 * sizeof(float);

int validate(const fmcw_cmap_config& c) {
  if (int rc = fmcw::check_map_dims(c.n_range, c.n_doppler)) return rc;
  if (c.n_streams < 1 || c.n_streams > 64) return fail(FMCW_EINVAL, "n_streams %u (1..64)", c.n_streams);
  if (!std::isfinite(c.gain) || !(c.gain > 0.f) || c.gain > 1.f)
    return fail(FMCW_EINVAL, "gain %g: must be finite, 0 < gain <= 1", c.gain);
  if (!std::isfinite(c.alpha) || !(c.alpha > 0.f)) return fail(FMCW_EINVAL, "alpha %g: must be finite and > 0", c.alpha);
  if (!std::isfinite(c.floor) || c.floor < 0.f) return fail(FMCW_EINVAL, "floor %g: must be finite and >= 0", c.floor);
  if (c.clip != 0.f && (!std::isfinite(c.clip) || c.clip < 1.f))
    return fail(FMCW_EINVAL, "clip %g: must be 0 (off), or finite and >= 1", c.clip);
  if (c.spread_range > (uint32_t)fmcw::kCmMaxSpread) return fail(FMCW_EINVAL, "spread_range %u (0..4)", c.spread_range);
  if (c.spread_doppler > (uint32_t)fmcw::kCmMaxSpread || 2 * c.spread_doppler + 1 > c.n_doppler)
    return fail(FMCW_EINVAL, "spread_doppler %u (0..4, 2 spread_doppler + 1 <= n_doppler)", c.spread_doppler);
  if (c.warmup < 1) return fail(FMCW_EINVAL, "warmup %u: must be >= 1", c.warmup);
  if (c.max_frames < c.n_streams || c.max_frames % c.n_streams != 0 ||
      (uint64_t)c.max_frames * c.n_range * c.n_doppler >= (1ull << 32))
    return fail(FMCW_EINVAL, "max_frames %u: need a multiple of n_streams %u, >= n_streams, and max_frames x cells < 2^32",
                c.max_frames, c.n_streams);
  if (int rc = fmcw::check_device_id(c.device_id)) return rc;
  for (int i = 0; i < 4; ++i)
    if (c.reserved[i] != 0) return fail(FMCW_EINVAL, "reserved[%d] = %u: must be 0", i, c.reserved[i]);
  return FMCW_OK;
}

using CmFn = void (*)(const float*, float*, const uint32_t*, fmcw::CmapArgs, int, uint32_t*, const uint32_t*, fmcw_det*,
                      uint32_t);

template <bool EMIT>
CmFn pick(uint32_t sd) {
  switch (sd) {
    case 0: return fmcw::k_cmap<EMIT, 0>;
    case 1: return fmcw::k_cmap<EMIT, 1>;
    case 2: return fmcw::k_cmap<EMIT, 2>;
    case 3: return fmcw::k_cmap<EMIT, 3>;
    default: return fmcw::k_cmap<EMIT, 4>;
  }
}

}  // namespace

struct fmcw_cmap {
  fmcw_cmap_config cfg;
  CmFn count = nullptr, emit = nullptr;   // the instantiations of this spread_doppler
  fmcw::CmapArgs args;
  size_t lds_bytes = 0;        // dynamic LDS of a k_cmap workgroup
  uint32_t max_grid = 1;       // workgroups resident at once (occupancy x CUs): the built-in bound
  uint32_t grid = 1;           // workgroups of the two passes at most (fmcw_cmap_set_grid_for_test)
  float* planes = nullptr;     // 2 copies x n_streams planes
  uint32_t* ctl = nullptr;     // current copy, its snapshot, ages[B], their snapshot[B]
  uint32_t* tile_words = nullptr;  // counts[max_tiles], offs[max_tiles]
  size_t max_tiles = 0;
  size_t plane_floats = 0;     // n_streams x cells
};

extern "C" {

void fmcw_cmap_config_default(fmcw_cmap_config* cfg) {
  if (!cfg) return;
  std::memset(cfg, 0, sizeof(*cfg));
  cfg->n_range = 1024;
  cfg->n_doppler = 128;
  cfg->n_streams = 1;
  cfg->gain = 0.125f;
  cfg->alpha = 4.0f;
  cfg->floor = 0.f;
  cfg->clip = 0.f;
  cfg->spread_range = 1;
  cfg->spread_doppler = 1;
  cfg->warmup = 8;
  cfg->max_frames = 1;
  cfg->device_id = 0;
}

int fmcw_cmap_destroy(fmcw_cmap* c) {
  if (!c) return FMCW_OK;
  fmcw::free_scratch(c->cfg.device_id, {c->planes, c->ctl, c->tile_words});
  delete c;
  return FMCW_OK;
}

int fmcw_cmap_create(const fmcw_cmap_config* cfg, fmcw_cmap** out) {
  if (!cfg || !out) return fail(FMCW_EINVAL, "null argument");
  *out = nullptr;
  int rc = validate(*cfg);
  if (rc) return rc;
  hipDeviceProp_t prop;
  if ((rc = fmcw::open_device(cfg->device_id, &prop))) return rc;

  fmcw_cmap* c = new fmcw_cmap();
  c->cfg = *cfg;
  fmcw::CmapArgs& a = c->args;
  const int nd = (int)cfg->n_doppler, ns = (int)cfg->n_range;
  a.ns = ns;
  a.lg_nd = __builtin_ctz(cfg->n_doppler);
  a.n_streams = (int)cfg->n_streams;
  a.sr = (int)cfg->spread_range;
  a.rows = std::min(fmcw::kCmTileCells / nd, ns);
  a.tiles_per_plane = ns / a.rows;
  a.gain = cfg->gain;
  a.alpha = cfg->alpha;
  a.floor = cfg->floor;
  a.clip = cfg->clip;
  a.warmup = cfg->warmup;
  c->max_tiles = (size_t)cfg->max_frames * (size_t)a.tiles_per_plane;
  c->plane_floats = (size_t)cfg->n_streams * (size_t)ns * (size_t)nd;
  c->lds_bytes = fmcw::cmap_lds_floats(nd, a.rows, a.sr) * sizeof(float);
  c->count = pick<false>(cfg->spread_doppler);
  c->emit = pick<true>(cfg->spread_doppler);
  const void* const count = reinterpret_cast<const void*>(c->count);
  const void* const emit = reinterpret_cast<const void*>(c->emit);
  if ((rc = fmcw::raise_lds_limit({count, emit}, kMaxLdsBytes, "k_cmap"))) {
    delete c;
    return rc;
  }
  c->max_grid = c->grid = fmcw::resident_grid(emit, fmcw::kCmNT, c->lds_bytes, prop);
  const size_t ctl_words = 2 + 2 * (size_t)cfg->n_streams;
  const size_t plane_bytes = 2 * c->plane_floats * sizeof(float), tile_bytes = 2 * c->max_tiles * sizeof(uint32_t);
  if (!fmcw::alloc_scratch({fmcw::scratch(c->planes, plane_bytes), fmcw::scratch(c->ctl, ctl_words * sizeof(uint32_t)),
                            fmcw::scratch(c->tile_words, tile_bytes)})) {
    fmcw_cmap_destroy(c);
    return fail(FMCW_ENOMEM, "hipMalloc for the clutter map's %zu B of planes and tile words failed",
                plane_bytes + tile_bytes);
  }
  // ages 0, copy 0 current; the planes' contents are irrelevant at age 0
  if (hipMemsetAsync(c->ctl, 0, ctl_words * sizeof(uint32_t), nullptr) != hipSuccess ||
      hipStreamSynchronize(nullptr) != hipSuccess) {
    (void)hipGetLastError();
    fmcw_cmap_destroy(c);
    return fail(FMCW_EHIP, "clearing the clutter map's ages at create");
  }
  *out = c;
  return FMCW_OK;
}

int fmcw_cmap_set_grid_for_test(fmcw_cmap* c, uint32_t grid) {
  if (!c) return fail(FMCW_EINVAL, "null clutter map");
  c->grid = fmcw::clamp_grid(grid, c->max_grid);
  return FMCW_OK;
}

int fmcw_cmap_reset(fmcw_cmap* c, void* stream) {
  if (!c) return fail(FMCW_EINVAL, "null clutter map");
  if (hipSetDevice(c->cfg.device_id) != hipSuccess) return fail(FMCW_EHIP, "hipSetDevice");
  if (hipMemsetAsync(c->ctl + 2, 0, c->cfg.n_streams * sizeof(uint32_t), reinterpret_cast<hipStream_t>(stream)) !=
      hipSuccess) {
    (void)hipGetLastError();
    return fail(FMCW_EHIP, "clearing the clutter map's ages");
  }
  return FMCW_OK;
}

static int state_copy(fmcw_cmap* c, bool set, float* planes_dev, uint32_t* ages_dev, void* stream) {
  if (int rc = fmcw::aligned(planes_dev, 16, "planes_dev")) return rc;
  if (int rc = fmcw::aligned(ages_dev, 4, "ages_dev")) return rc;
  if (hipSetDevice(c->cfg.device_id) != hipSuccess) return fail(FMCW_EHIP, "hipSetDevice");
  const size_t n4 = c->plane_floats / 4;
  const uint32_t blocks = planes_dev ? (uint32_t)std::min<size_t>((n4 + 255) / 256, 4096) : 1u;
  hipLaunchKernelGGL(set ? fmcw::k_cmap_state<true> : fmcw::k_cmap_state<false>, dim3(blocks), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), c->planes, c->ctl, planes_dev, ages_dev,
                     (int)c->cfg.n_streams, n4);
  return fmcw::check_launch("k_cmap_state");
}

int fmcw_cmap_get_state(fmcw_cmap* c, float* planes_dev, uint32_t* ages_dev, void* stream) {
  if (!c) return fail(FMCW_EINVAL, "null clutter map");
  if (!planes_dev && !ages_dev) return fail(FMCW_EINVAL, "null planes_dev and null ages_dev: nothing to copy");
  return state_copy(c, false, planes_dev, ages_dev, stream);
}

int fmcw_cmap_set_state(fmcw_cmap* c, const float* planes_dev, const uint32_t* ages_dev, void* stream) {
  if (!c) return fail(FMCW_EINVAL, "null clutter map");
  if (!planes_dev) return fail(FMCW_EINVAL, "null planes_dev: the ages cannot be set without the planes they describe");
  return state_copy(c, true, const_cast<float*>(planes_dev), const_cast<uint32_t*>(ages_dev), stream);
}

int fmcw_cmap_enqueue(fmcw_cmap* c, const float* map_dev, size_t n_frames, fmcw_det* dets_dev, size_t det_cap,
                      uint32_t* n_dets_dev, void* stream) {
  if (!c) return fail(FMCW_EINVAL, "null clutter map");
  if (!n_dets_dev) return fail(FMCW_EINVAL, "null n_dets_dev");
  if (n_frames > c->cfg.max_frames)
    return fail(FMCW_EINVAL, "n_frames %zu exceeds max_frames %u", n_frames, c->cfg.max_frames);
  if (n_frames % c->cfg.n_streams != 0)
    return fail(FMCW_EINVAL, "n_frames %zu is not a multiple of n_streams %u", n_frames, c->cfg.n_streams);
  if (int rc = fmcw::check_map_and_dets(map_dev, n_frames, dets_dev, det_cap)) return rc;
  if (hipSetDevice(c->cfg.device_id) != hipSuccess) return fail(FMCW_EHIP, "hipSetDevice");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int n_scans = (int)(n_frames / c->cfg.n_streams);
  const int n_tiles = (int)(n_frames * (size_t)c->args.tiles_per_plane);
  const uint32_t n_units = c->cfg.n_streams * (uint32_t)c->args.tiles_per_plane;
  uint32_t* const counts = c->tile_words;
  uint32_t* const offs = c->tile_words + c->max_tiles;
  const uint32_t n_wg = std::min(n_units, c->grid);
  // every index fits 32 bits: max_frames x cells < 2^32
  const uint32_t cap = (uint32_t)std::min<size_t>(det_cap, 0xffffffffu);
  if (n_scans) {
    hipLaunchKernelGGL(c->count, dim3(n_wg), dim3(fmcw::kCmNT), c->lds_bytes, s, map_dev, c->planes,
                       static_cast<const uint32_t*>(c->ctl), c->args, n_scans, counts,
                       static_cast<const uint32_t*>(nullptr), static_cast<fmcw_det*>(nullptr), 0u);
    if (int rc = fmcw::check_launch("k_cmap count")) return rc;
  }
  hipLaunchKernelGGL(fmcw::k_cmap_scan, dim3(1), dim3(fmcw::kCmScanNT), 0, s, static_cast<const uint32_t*>(counts), offs,
                     n_tiles, n_dets_dev, c->ctl, (int)c->cfg.n_streams, (uint32_t)n_scans);
  if (int rc = fmcw::check_launch("k_cmap_scan")) return rc;
  if (n_scans) {   // whatever det_cap is: this pass also writes the state
    hipLaunchKernelGGL(c->emit, dim3(n_wg), dim3(fmcw::kCmNT), c->lds_bytes, s, map_dev, c->planes,
                       static_cast<const uint32_t*>(c->ctl), c->args, n_scans, static_cast<uint32_t*>(nullptr),
                       static_cast<const uint32_t*>(offs), dets_dev, cap);
    if (int rc = fmcw::check_launch("k_cmap emit")) return rc;
  }
  return FMCW_OK;
}

}  // extern "C"
