// fmcw_tws_dev.hip -- the device track-while-scan tracker of include/fmcw.h (fmcw_tws_dev_*): a
// device-resident record list (detections or plots) in, per (scan, stream) the firm and coasting tracks
// and the two counts out.  The arithmetic is the host tracker's (tws_tracker.cpp); the kernels and the
// wave mapping are described in tws_dev_kernel.hpp.
//
// Two launches per call, nothing allocated, no synchronisation, no word that has to be cleared between
// calls: k_frame_index (rec_tiles.hpp) writes every start word the tracker reads, and k_tws_track (the last kernel) also
// writes the two status words.  The track files live in the handle's state block and persist from call
// to call; fmcw_tws_dev_reset puts them back to power-up in stream order.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "internal.hpp"
#include "tws_dev_kernel.hpp"

using fmcw::fail;

static_assert(sizeof(fmcw_tws_config) == 36 && sizeof(fmcw_tws_dev_config) == 48, "fmcw.h device tracker layout");
static_assert(sizeof(fmcw_track) == 28 && sizeof(fmcw_det) == 16 && sizeof(fmcw_plot) == 32, "fmcw.h record layouts");

namespace {

using namespace fmcw_twsd;

int validate(const fmcw_tws_dev_config& c) {
  const fmcw_tws_config& t = c.tws;
  if (t.max_tracks < 1 || t.max_tracks > 64) return fail(FMCW_EINVAL, "max_tracks %u (1..64)", t.max_tracks);
  if (t.max_dets < 1 || t.max_dets > 64) return fail(FMCW_EINVAL, "max_dets %u (1..64)", t.max_dets);
  if (t.alpha_q8 > 255) return fail(FMCW_EINVAL, "alpha_q8 %u (0..255)", t.alpha_q8);
  if (t.beta_q8 > 255) return fail(FMCW_EINVAL, "beta_q8 %u (0..255)", t.beta_q8);
  if (t.gate_r > 4096) return fail(FMCW_EINVAL, "gate_r %u (0..4096)", t.gate_r);
  if (t.gate_d > 4096) return fail(FMCW_EINVAL, "gate_d %u (0..4096)", t.gate_d);
  if (c.n_streams < 1 || c.n_streams > 4096) return fail(FMCW_EINVAL, "n_streams %u (1..4096)", c.n_streams);
  if (c.max_scans < 1 || (uint64_t)c.max_scans * c.n_streams >= (1ull << 31))
    return fail(FMCW_EINVAL, "max_scans %u: need 1 <= max_scans and max_scans x n_streams < 2^31", c.max_scans);
  if (int rc = fmcw::check_device_id(c.device_id)) return rc;
  return FMCW_OK;
}

}  // namespace

struct fmcw_tws_dev {
  fmcw_tws_dev_config cfg;
  uint32_t grid = 0;          // workgroups of both kernels at most (fmcw_tws_dev_set_grid_for_test); 0: built-in
  uint32_t* state = nullptr;  // n_streams x kStateWords
  uint32_t* start = nullptr;  // max_scans x n_streams + 1
};

extern "C" {

void fmcw_tws_dev_config_default(fmcw_tws_dev_config* cfg) {
  if (!cfg) return;
  fmcw_tws_config_default(&cfg->tws);
  cfg->n_streams = 1;
  cfg->max_scans = 1024;
  cfg->device_id = 0;
}

int fmcw_tws_dev_create(const fmcw_tws_dev_config* cfg, fmcw_tws_dev** out) {
  if (!cfg || !out) return fail(FMCW_EINVAL, "null argument");
  *out = nullptr;
  int rc = validate(*cfg);
  if (rc) return rc;
  if ((rc = fmcw::open_device(cfg->device_id))) return rc;
  fmcw_tws_dev* t = new fmcw_tws_dev();
  t->cfg = *cfg;
  const size_t state_bytes = (size_t)cfg->n_streams * kStateWords * sizeof(uint32_t);
  const size_t start_bytes = ((size_t)cfg->max_scans * cfg->n_streams + 1) * sizeof(uint32_t);
  if (!fmcw::alloc_scratch({fmcw::scratch(t->state, state_bytes), fmcw::scratch(t->start, start_bytes)})) {
    fmcw_tws_dev_destroy(t);
    return fail(FMCW_ENOMEM, "hipMalloc(%zu + %zu) for the tracker's state and frame index failed", state_bytes,
                start_bytes);
  }
  // power-up state, complete before create returns
  if (fmcw_tws_dev_reset(t, nullptr) != FMCW_OK || hipStreamSynchronize(nullptr) != hipSuccess) {
    (void)hipGetLastError();
    fmcw_tws_dev_destroy(t);
    return fail(FMCW_EHIP, "k_tws_reset at create");
  }
  *out = t;
  return FMCW_OK;
}

int fmcw_tws_dev_destroy(fmcw_tws_dev* t) {
  if (!t) return FMCW_OK;
  fmcw::free_scratch(t->cfg.device_id, {t->state, t->start});
  delete t;
  return FMCW_OK;
}

int fmcw_tws_dev_reset(fmcw_tws_dev* t, void* stream) {
  if (!t) return fail(FMCW_EINVAL, "null tracker");
  if (hipSetDevice(t->cfg.device_id) != hipSuccess) return fail(FMCW_EHIP, "hipSetDevice");
  const uint32_t blocks = std::min<uint32_t>(1024u, (t->cfg.n_streams * kStateWords + 255u) / 256u);
  hipLaunchKernelGGL(k_tws_reset, dim3(blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), t->state,
                     t->cfg.n_streams);
  return fmcw::check_launch("k_tws_reset");
}

int fmcw_tws_dev_set_grid_for_test(fmcw_tws_dev* t, uint32_t grid) {
  if (!t) return fail(FMCW_EINVAL, "null tracker");
  t->grid = grid;
  return FMCW_OK;
}

int fmcw_tws_dev_enqueue(fmcw_tws_dev* t, const void* recs_dev, size_t rec_stride, size_t rec_cap,
                         const uint32_t* n_recs_dev, size_t n_scans, fmcw_track* tracks_dev, size_t track_cap,
                         uint32_t* counts_dev, uint32_t* status_dev, void* stream) {
  // the checks that need no tracker come first, so that they hold without a device
  if (rec_stride != sizeof(fmcw_det) && rec_stride != sizeof(fmcw_plot))
    return fail(FMCW_EINVAL, "rec_stride %zu (16: fmcw_det, 32: fmcw_plot)", rec_stride);
  if (track_cap < 1) return fail(FMCW_EINVAL, "track_cap %zu (>= 1)", track_cap);
  if (rec_cap && !recs_dev) return fail(FMCW_EINVAL, "null recs_dev with rec_cap %zu", rec_cap);
  if (int rc = fmcw::aligned(recs_dev, 4, "recs_dev")) return rc;
  if (!n_recs_dev) return fail(FMCW_EINVAL, "null n_recs_dev");
  if (!status_dev) return fail(FMCW_EINVAL, "null status_dev");
  if (n_scans && !tracks_dev) return fail(FMCW_EINVAL, "null tracks_dev with n_scans %zu", n_scans);
  if (n_scans && !counts_dev) return fail(FMCW_EINVAL, "null counts_dev with n_scans %zu", n_scans);
  if (int rc = fmcw::aligned(tracks_dev, 4, "tracks_dev")) return rc;
  if (!t) return fail(FMCW_EINVAL, "null tracker");
  if (n_scans > t->cfg.max_scans) return fail(FMCW_EINVAL, "n_scans %zu exceeds max_scans %u", n_scans, t->cfg.max_scans);
  if (hipSetDevice(t->cfg.device_id) != hipSuccess) return fail(FMCW_EHIP, "hipSetDevice");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const uint32_t cap = (uint32_t)std::min<size_t>(rec_cap, kMaxRecs);   // n = min(n_recs_dev[0], cap)
  const uint32_t n_streams = t->cfg.n_streams;
  const uint32_t n_groups = (uint32_t)n_scans * n_streams;               // < 2^31 (validate)
  const uint8_t* recs = static_cast<const uint8_t*>(recs_dev);
  const uint32_t tiles = cap / kIdxTile + 1;
  const uint32_t gi = std::min(tiles, fmcw::clamp_grid(t->grid, kIdxMaxGrid));
  hipLaunchKernelGGL((fmcw_rec::k_frame_index<kIdxThreads, kIdxPer, false>), dim3(gi), dim3(kIdxThreads), 0, s, recs,
                     (uint32_t)rec_stride, cap, n_recs_dev, n_groups, t->start);
  if (int rc = fmcw::check_launch("k_frame_index")) return rc;
  const uint32_t wgs = (n_streams + kTrackWaves - 1) / kTrackWaves;   // one wave per stream
  const uint32_t gt = n_scans ? std::min(wgs, fmcw::clamp_grid(t->grid, kTrackMaxGrid)) : 1u;
  auto track = t->cfg.tws.rtl_compat ? k_tws_track<true> : k_tws_track<false>;
  hipLaunchKernelGGL(track, dim3(gt), dim3(64 * kTrackWaves), 0, s, recs, (uint32_t)rec_stride, cap, n_recs_dev,
                     static_cast<const uint32_t*>(t->start), (uint32_t)n_scans, n_streams, t->cfg.tws, t->state,
                     reinterpret_cast<uint32_t*>(tracks_dev), track_cap, counts_dev, status_dev);
  return fmcw::check_launch("k_tws_track");
}

}  // extern "C"
