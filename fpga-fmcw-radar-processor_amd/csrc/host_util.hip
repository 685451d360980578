// host_util.hip -- the helpers of internal.hpp that the objects beside fmcw_handle share (plotter, bearing
// estimator, beamformer, cell-averaging detector, device tracker, clutter map, adaptive weights, merger,
// unfolder, exciser).  Host code only.
#include <cstring>

#include "internal.hpp"

namespace fmcw {

int check_map_dims(uint32_t n_range, uint32_t n_doppler) {
  if (!pow2(n_range) || n_range < 64 || n_range > 8192)
    return fail(FMCW_EINVAL, "n_range=%u: must be a power of two in [64, 8192]", n_range);
  if (!pow2(n_doppler) || n_doppler < 32 || n_doppler > 1024)
    return fail(FMCW_EINVAL, "n_doppler=%u: must be a power of two in [32, 1024]", n_doppler);
  return FMCW_OK;
}

int check_device_id(int device_id) {
  if (device_id < 0 || device_id > 63) return fail(FMCW_EINVAL, "device_id %d (0..63)", device_id);
  return FMCW_OK;
}

int check_n_rx(uint32_t n_rx, uint32_t max) {
  if (n_rx >= 1 && n_rx <= max) return FMCW_OK;
  if (max < 64) return fail(FMCW_EINVAL, "n_rx=%u: must be in [1, %u] (%u..64 is not built)", n_rx, max, max + 1);
  return fail(FMCW_EINVAL, "n_rx=%u: must be in [1, %u]", n_rx, max);
}

int check_float_window(int window, const char* object) {
  if (window == FMCW_WIN_NONE || window == FMCW_WIN_HAMMING) return FMCW_OK;
  return fail(FMCW_EINVAL, "window %d: the %s has the float windows only (NONE, HAMMING)", window, object);
}

int check_mti_mode(int mti_mode) {
  if (mti_mode == FMCW_MTI_OFF || mti_mode == FMCW_MTI_2PULSE || mti_mode == FMCW_MTI_3PULSE) return FMCW_OK;
  return fail(FMCW_EINVAL, "mti_mode %d (0, 2, 3)", mti_mode);
}

int open_device(int device_id, hipDeviceProp_t* prop) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) {
    (void)hipGetLastError();
    return fail(FMCW_ENODEV, "no HIP device");
  }
  if (device_id >= ndev) return fail(FMCW_ENODEV, "device_id %d out of range", device_id);
  hipDeviceProp_t p;
  if (hipSetDevice(device_id) != hipSuccess || hipGetDeviceProperties(&p, device_id) != hipSuccess) {
    (void)hipGetLastError();
    return fail(FMCW_ENODEV, "device_id %d", device_id);
  }
  if (std::strncmp(p.gcnArchName, "gfx950", 6) != 0)
    return fail(FMCW_ENODEV, "device %d is %s; this build targets gfx950 (MI355X)", device_id, p.gcnArchName);
  if (prop) *prop = p;
  return FMCW_OK;
}

int aligned(const void* p, unsigned bytes, const char* name) {
  if (reinterpret_cast<uintptr_t>(p) & (bytes - 1u)) return fail(FMCW_EINVAL, "%s must be %u-byte aligned", name, bytes);
  return FMCW_OK;
}

int check_map_and_dets(const float* map_dev, size_t n_frames, const fmcw_det* dets_dev, size_t det_cap) {
  if (n_frames && !map_dev) return fail(FMCW_EINVAL, "null map_dev with n_frames %zu", n_frames);
  if (int rc = aligned(map_dev, 16, "map_dev")) return rc;
  if (!dets_dev && det_cap) return fail(FMCW_EINVAL, "null dets_dev with det_cap %zu", det_cap);
  return aligned(dets_dev, 16, "dets_dev");
}

int check_rec_list_args(const void* recs_dev, size_t rec_stride, size_t rec_cap, const uint32_t* n_recs_dev,
                        const void* out_dev, size_t out_cap, const uint32_t* status_dev) {
  if (rec_stride != 16 && rec_stride != 32) return fail(FMCW_EINVAL, "rec_stride %zu (16 or 32)", rec_stride);
  if (rec_cap && !recs_dev) return fail(FMCW_EINVAL, "null recs_dev with rec_cap %zu", rec_cap);
  if (!n_recs_dev) return fail(FMCW_EINVAL, "null n_recs_dev");
  if (out_cap && !out_dev) return fail(FMCW_EINVAL, "null out_dev with out_cap %zu", out_cap);
  if (!status_dev) return fail(FMCW_EINVAL, "null status_dev");
  if (int rc = aligned(recs_dev, 16, "recs_dev")) return rc;
  return aligned(out_dev, 16, "out_dev");
}

bool alloc_scratch(std::initializer_list<ScratchBuf> bufs) {
  for (const ScratchBuf& b : bufs)
    if (hipMalloc(b.ptr, b.bytes) != hipSuccess) {
      (void)hipGetLastError();
      return false;
    }
  return true;
}

void free_scratch(int device_id, std::initializer_list<void*> ptrs) {
  hipSetDevice(device_id);
  for (void* p : ptrs)
    if (p) hipFree(p);
}

bool upload_tables(std::initializer_list<TableUpload> tables) {
  for (const TableUpload& t : tables)
    if (hipMemcpy(t.dst, t.src, t.bytes, hipMemcpyHostToDevice) != hipSuccess) {
      (void)hipGetLastError();
      return false;
    }
  return true;
}

int raise_lds_limit(std::initializer_list<const void*> fns, size_t bytes, const char* name) {
  for (const void* fn : fns)
    if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess) {
      (void)hipGetLastError();
      return fail(FMCW_EHIP, "%s: %zu B of LDS per workgroup refused", name, bytes);
    }
  return FMCW_OK;
}

uint32_t resident_grid(const void* fn, int threads, size_t lds_bytes, const hipDeviceProp_t& prop) {
  int per_cu = 1;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, threads, lds_bytes) != hipSuccess || per_cu < 1) {
    (void)hipGetLastError();
    per_cu = 1;
  }
  return (uint32_t)per_cu * (uint32_t)std::max(prop.multiProcessorCount, 1);
}

}  // namespace fmcw
