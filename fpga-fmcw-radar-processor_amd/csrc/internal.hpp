// internal.hpp -- what the host translation units of libfmcw.so share: the error plumbing (fmcw_api.hip)
// and the helpers of the objects beside fmcw_handle (host_util.hip): device opening, argument checks,
// grid sizing.  Free functions; every object keeps its own handle struct.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <initializer_list>
#include <type_traits>
#include <vector>

#include "../../include/fmcw.h"

namespace fmcw {

// Sets the calling thread's fmcw_last_error() message (printf format; the one thread-local
// string lives in fmcw_api.hip) and returns `code`.
int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
// FMCW_OK, or FMCW_EHIP with the pending launch error of kernel `what`
int check_launch(const char* what);
// The fp32 window table of n points the kernels multiply by (fmcw_api.hip): FMCW_WIN_HAMMING, or
// ones for FMCW_WIN_NONE, scaled by 2^-shift; FMCW_WIN_Q15_RTL gives the ROM integers.
std::vector<float> window_table(uint32_t n, int kind, uint32_t shift = 0);

inline bool pow2(uint32_t x) { return x && !(x & (x - 1)); }
// a *_set_grid_for_test value against the built-in bound: 0 means the bound
inline uint32_t clamp_grid(uint32_t grid, uint32_t max_grid) { return grid ? std::min(max_grid, grid) : max_grid; }

// Every function below returns FMCW_OK, or the code of the fail() whose message it has set.

// n_range a power of two in [64, 8192], n_doppler one in [32, 1024]: the maps the stage kernels write
int check_map_dims(uint32_t n_range, uint32_t n_doppler);
int check_device_id(int device_id);   // 0..63
// The configuration checks of the objects on fmcw_range_ct's plain spectrum (bearing estimator,
// beamformer, adaptive weights).  The interface's n_rx bound is 64; a smaller `max` is what is built.
int check_n_rx(uint32_t n_rx, uint32_t max);             // 1..max
int check_float_window(int window, const char* object);  // NONE, HAMMING; "the <object> has ..."
int check_mti_mode(int mti_mode);                        // fmcw_mti_mode
// f(std::integral_constant<int, M>{}), M the fmcw_mti_mode of a checked mti_mode: how a run-time mode
// picks a kernel's MTI instantiation.  f returns the same type for every M.
template <class F>
auto with_mti(int mti_mode, F&& f) {
  if (mti_mode == FMCW_MTI_2PULSE) return f(std::integral_constant<int, FMCW_MTI_2PULSE>{});
  if (mti_mode == FMCW_MTI_3PULSE) return f(std::integral_constant<int, FMCW_MTI_3PULSE>{});
  return f(std::integral_constant<int, FMCW_MTI_OFF>{});
}
// Makes device_id (>= 0: check_device_id) the current device; FMCW_ENODEV unless it exists and is a
// gfx950.  *prop, when given, receives its properties.
int open_device(int device_id, hipDeviceProp_t* prop = nullptr);
// "<name> must be <bytes>-byte aligned"; a null p passes
int aligned(const void* p, unsigned bytes, const char* name);
// What the detectors' enqueue ask of their map and their list, in this order: map_dev present (with
// n_frames) and 16-byte aligned, dets_dev present (with det_cap) and 16-byte aligned.
int check_map_and_dets(const float* map_dev, size_t n_frames, const fmcw_det* dets_dev, size_t det_cap);
// What the enqueue of a list-in / list-out object (merger, unfolder) asks of its arguments before it
// looks at the object, in this order: rec_stride 16 or 32, recs_dev (with rec_cap), n_recs_dev, out_dev
// (with out_cap) and status_dev present, recs_dev and out_dev 16-byte aligned.
int check_rec_list_args(const void* recs_dev, size_t rec_stride, size_t rec_cap, const uint32_t* n_recs_dev,
                        const void* out_dev, size_t out_cap, const uint32_t* status_dev);

// An object's device scratch: alloc_scratch() fills every pointer of the list or returns false with the
// pending HIP error cleared (the caller then destroys the object and reports FMCW_ENOMEM with its own
// text); free_scratch() makes the object's device current and frees those that are set.
struct ScratchBuf {
  void** ptr;
  size_t bytes;
};
template <class T>
ScratchBuf scratch(T*& p, size_t bytes) { return {reinterpret_cast<void**>(&p), bytes}; }
bool alloc_scratch(std::initializer_list<ScratchBuf> bufs);
void free_scratch(int device_id, std::initializer_list<void*> ptrs);
// The host tables an object copies to its scratch at create (window, twiddles, weights), in list order:
// false with the pending HIP error cleared (the caller destroys the object and reports FMCW_EHIP).
struct TableUpload {
  void* dst;
  const void* src;
  size_t bytes;
};
bool upload_tables(std::initializer_list<TableUpload> tables);

// The sizes of one call on a record list, for kernels that stride over tiles of `tile` items:
// cap = min(rec_cap, max_recs) records examined at most; tiles of its cap x items_per_rec items;
// workgroups of the tile kernels; workgroups of the frame index, whose cap + 1 items are one tile more
// than the records' when cap is a multiple of the tile.  `grid`: the object's bound (clamp_grid).
inline uint32_t tiles_of(uint64_t items, uint32_t tile) { return (uint32_t)((items + tile - 1) / tile); }
struct ListPlan {
  uint32_t cap, tiles, grid, index_grid;
};
inline ListPlan plan_list(size_t rec_cap, uint32_t max_recs, uint32_t items_per_rec, uint32_t tile, uint32_t grid) {
  ListPlan p;
  p.cap = (uint32_t)std::min<size_t>(rec_cap, max_recs);   // n = min(n_recs_dev[0], cap)
  p.tiles = tiles_of((uint64_t)p.cap * items_per_rec, tile);   // <= the tiles the scratch was sized for
  p.grid = std::min(p.tiles, grid);
  p.index_grid = std::min(p.cap / tile + 1, grid);
  return p;
}

// hipFuncAttributeMaxDynamicSharedMemorySize = bytes on each kernel of `fns` ("<name>: .. refused").
// The attribute is per kernel, not per object: pass the largest any configuration needs, so that it
// does not shrink when a second object is created.
int raise_lds_limit(std::initializer_list<const void*> fns, size_t bytes, const char* name);

// Workgroups of `fn` resident at once: occupancy x CUs, 1 per CU where the runtime gives no answer.
uint32_t resident_grid(const void* fn, int threads, size_t lds_bytes, const hipDeviceProp_t& prop);

}  // namespace fmcw

#define HIP_TRY(expr)                                                                          \
  do {                                                                                         \
    hipError_t e_ = (expr);                                                                    \
    if (e_ != hipSuccess) return fmcw::fail(FMCW_EHIP, "%s: %s (%s:%d)", #expr,                \
                                            hipGetErrorString(e_), __FILE__, __LINE__);        \
  } while (0)
