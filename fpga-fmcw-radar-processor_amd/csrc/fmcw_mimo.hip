// fmcw_mimo.hip -- the TDM-MIMO virtual array of include/fmcw.h: the corner-turned spectrum of
// fmcw_range_ct for n_chirps = n_tx * n_d chirps in, a spectrum of n_tx * n_rx channels and n_d chirps out,
// every transmitter's sequence delayed to TX 0's sampling instants.
//
// One persistent launch per call (mimo_kernel.hpp's k_mimo): a wave per tile of 1024 input points, read
// once and written once.  The ramp comes from v_sin / v_cos at launch; the object owns no device memory.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "internal.hpp"
#include "mimo_kernel.hpp"

using fmcw::fail;

static_assert(sizeof(fmcw_mimo_config) == 32, "fmcw.h virtual array layout");

namespace {

using MimoFn = void (*)(const float2*, float2*, int, int, int, int);

// ALIGN_DFT with one transmitter has the unit ramp: the copy is its result
template <int ND>
MimoFn pick_align(bool dft) {
  if constexpr (ND < 1024) {
    if (dft) return fmcw::k_mimo<ND, true>;
  }
  return fmcw::k_mimo<ND, false>;   // n_d = 1024 leaves one transmitter only
}

MimoFn pick(uint32_t nd, bool dft) {
  switch (nd) {
    case 32: return pick_align<32>(dft);
    case 64: return pick_align<64>(dft);
    case 128: return pick_align<128>(dft);
    case 256: return pick_align<256>(dft);
    case 512: return pick_align<512>(dft);
    default: return pick_align<1024>(dft);
  }
}

int ilog2(uint32_t x) {
  int n = 0;
  while (x >>= 1) ++n;
  return n;
}

int validate(const fmcw_mimo_config& c) {
  if (!fmcw::pow2(c.n_range) || c.n_range < 64 || c.n_range > 8192)
    return fail(FMCW_EINVAL, "n_range=%u: must be a power of two in [64, 8192]", c.n_range);
  if (!fmcw::pow2(c.n_chirps) || c.n_chirps < 32 || c.n_chirps > 1024)
    return fail(FMCW_EINVAL, "n_chirps=%u: must be a power of two in [32, 1024]", c.n_chirps);
  if (int rc = fmcw::check_n_rx(c.n_rx, 64)) return rc;
  if (!fmcw::pow2(c.n_tx) || c.n_tx > 32) return fail(FMCW_EINVAL, "n_tx=%u: must be a power of two in [1, 32]", c.n_tx);
  if (c.n_chirps / c.n_tx < 32)
    return fail(FMCW_EINVAL, "n_tx=%u: n_d = n_chirps / n_tx = %u, must be at least 32", c.n_tx, c.n_chirps / c.n_tx);
  if (c.n_tx * c.n_rx > 64)
    return fail(FMCW_EINVAL, "n_tx=%u x n_rx=%u: at most 64 virtual channels", c.n_tx, c.n_rx);
  if (c.align != FMCW_MIMO_ALIGN_NONE && c.align != FMCW_MIMO_ALIGN_DFT)
    return fail(FMCW_EINVAL, "align %d (0 NONE, 1 DFT)", c.align);
  if (c.reserved[0] != 0 || c.reserved[1] != 0)
    return fail(FMCW_EINVAL, "reserved {%u, %u}: must be 0", c.reserved[0], c.reserved[1]);
  if (int rc = fmcw::check_device_id(c.device_id)) return rc;
  return FMCW_OK;
}

}  // namespace

struct fmcw_mimo {
  fmcw_mimo_config cfg;
  MimoFn fn = nullptr;
  uint32_t max_grid = 1;   // workgroups resident at once (occupancy x CUs): the built-in bound
  uint32_t grid = 1;       // workgroups at most (fmcw_mimo_set_grid_for_test)
};

extern "C" {

void fmcw_mimo_config_default(fmcw_mimo_config* cfg) {
  if (!cfg) return;
  cfg->n_range = 1024;
  cfg->n_chirps = 128;
  cfg->n_rx = 4;
  cfg->n_tx = 2;
  cfg->align = FMCW_MIMO_ALIGN_DFT;
  cfg->reserved[0] = cfg->reserved[1] = 0;
  cfg->device_id = 0;
}

int fmcw_mimo_create(const fmcw_mimo_config* cfg, fmcw_mimo** out) {
  if (!cfg || !out) return fail(FMCW_EINVAL, "null argument");
  *out = nullptr;
  int rc = validate(*cfg);
  if (rc) return rc;
  hipDeviceProp_t prop;
  if ((rc = fmcw::open_device(cfg->device_id, &prop))) return rc;
  fmcw_mimo* m = new fmcw_mimo();
  m->cfg = *cfg;
  m->fn = pick(cfg->n_chirps / cfg->n_tx, cfg->align == FMCW_MIMO_ALIGN_DFT && cfg->n_tx > 1);
  m->max_grid = m->grid = fmcw::resident_grid(reinterpret_cast<const void*>(m->fn), fmcw::kMimoNT, 0, prop);
  *out = m;
  return FMCW_OK;
}

int fmcw_mimo_destroy(fmcw_mimo* m) {
  delete m;
  return FMCW_OK;
}

int fmcw_mimo_set_grid_for_test(fmcw_mimo* m, uint32_t grid) {
  if (!m) return fail(FMCW_EINVAL, "null virtual array");
  m->grid = fmcw::clamp_grid(grid, m->max_grid);
  return FMCW_OK;
}

int fmcw_mimo_enqueue(fmcw_mimo* m, const void* spec_dev, size_t n_frames, void* out_dev, void* stream) {
  if (!m) return fail(FMCW_EINVAL, "null virtual array");
  if (n_frames == 0) return FMCW_OK;
  if (!spec_dev || !out_dev) return fail(FMCW_EINVAL, "null spec_dev or out_dev with n_frames %zu", n_frames);
  if (int rc = fmcw::aligned(out_dev, 16, "out_dev")) return rc;
  if (int rc = fmcw::aligned(spec_dev, 16, "spec_dev")) return rc;
  const fmcw_mimo_config& c = m->cfg;
  const size_t rows_frame = (size_t)c.n_rx * c.n_range;
  if (n_frames > 0x7fffffffu / rows_frame)
    return fail(FMCW_EINVAL, "n_frames %zu: more than 2^31 - 1 spectrum rows (%zu per frame)", n_frames, rows_frame);
  const size_t bytes = n_frames * rows_frame * c.n_chirps * sizeof(float2);
  const uintptr_t src = reinterpret_cast<uintptr_t>(spec_dev), dst = reinterpret_cast<uintptr_t>(out_dev);
  if (src < dst + bytes && dst < src + bytes) return fail(FMCW_EINVAL, "out_dev overlaps spec_dev: they must be disjoint");
  if (hipSetDevice(c.device_id) != hipSuccess) return fail(FMCW_EHIP, "hipSetDevice");
  // n_range x n_chirps >= 64 x 32 points: a frame is a whole number of tiles, a tile lies in one (frame, rx)
  const int n_tiles = (int)(bytes / sizeof(float2) / fmcw::kMimoTile);
  const uint32_t n_wg = std::min((uint32_t)(((int64_t)n_tiles + fmcw::kMimoWPB - 1) / fmcw::kMimoWPB), m->grid);
  hipLaunchKernelGGL(m->fn, dim3(n_wg), dim3(fmcw::kMimoNT), 0, reinterpret_cast<hipStream_t>(stream),
                     static_cast<const float2*>(spec_dev), static_cast<float2*>(out_dev), ilog2(c.n_tx), (int)c.n_rx,
                     ilog2(c.n_range), n_tiles);
  return fmcw::check_launch("k_mimo");
}

}  // extern "C"
