"""Cell-averaging CFAR: CA, greatest-of and smallest-of (ctypes over fmcw_cacfar_*, include/fmcw.h).

The reference's detectors are ordered-statistic (RadarCore's "os1d" / "os2d"), whose cost follows the
data.  ``CaCfar`` is the detector whose cost does not: the same sums on every cell of a range-Doppler
map, two reads of the map per call.  It takes the maps ``RadarCore`` (``cfar="none"``) or
``BeamFormer`` write, and gives the same ``DET_DTYPE`` list and status words as ``RadarCore.cfar``, so
``PlotExtractor``, ``BearingEstimator`` and the gather take its output unchanged.  The window, the
canonical order of the sums and the thresholds are specified in include/fmcw.h.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from .radar_core import DET_DTYPE, DeviceBuffer, _ptr

_MODES = {"ca": L.CACFAR_CA, "go": L.CACFAR_GO, "so": L.CACFAR_SO}


class CaCfar:
    def __init__(self, N_RANGE: int = 1024, N_DOPPLER: int = 128, mode: str = "ca", ref=(4, 4), guard=(1, 2),
                 alpha: float = 4.0, max_frames: int = 1, device: int = 0):
        """mode: "ca" (T = alpha x mean of the window), "go" / "so" (alpha x the larger / smaller of the
        two half-window means).  ref, guard: (range, doppler) extents, 0..8 and 0..4."""
        self._lib = L.load()
        cfg = L.FmcwCaCfarConfig()
        self._lib.fmcw_cacfar_config_default(C.byref(cfg))
        cfg.n_range, cfg.n_doppler = N_RANGE, N_DOPPLER
        cfg.mode = _MODES[mode] if isinstance(mode, str) else mode
        cfg.ref_range, cfg.ref_doppler = ref
        cfg.guard_range, cfg.guard_doppler = guard
        cfg.alpha = alpha
        cfg.max_frames, cfg.device_id = max_frames, device
        self.cfg = cfg
        self.device = device
        h = C.c_void_p()
        L.check(self._lib.fmcw_cacfar_create(C.byref(cfg), C.byref(h)))
        self._h = h

    def map_frame_bytes(self) -> int:
        return self.cfg.n_range * self.cfg.n_doppler * 4

    def enqueue(self, maps, n_frames: int, dets, det_cap: int, n_dets, stream: int = 0):
        """Asynchronous, device pointers only (DeviceBuffer / torch CUDA tensors / ints).  maps: n_frames
        float32 maps; dets: room for det_cap records (None with det_cap 0 counts only); n_dets:
        FMCW_STATUS_WORDS (4) uint32 device words, [0] = detections found (may exceed det_cap)."""
        def p(x):
            return x if isinstance(x, int) or x is None else _ptr(x)[0]
        L.check(self._lib.fmcw_cacfar_enqueue(self._h, p(maps), n_frames, p(dets), det_cap, p(n_dets), stream or None))

    def detect(self, maps, det_cap: int | None = None) -> np.ndarray:
        """Synchronous.  maps: a host float32 array [frame][range][doppler] (or one map), or a
        DeviceBuffer / CUDA tensor holding whole maps.  Returns the DET_DTYPE list; reruns once with the
        reported count when the first capacity was short."""
        own = []
        try:
            if isinstance(maps, np.ndarray):
                host = np.ascontiguousarray(maps, dtype=np.float32)
                nbytes = host.nbytes
                maps = DeviceBuffer(max(nbytes, 16), self.device)
                own.append(maps)
                if nbytes:
                    maps.upload(host)
            else:
                nbytes = maps.nbytes if isinstance(maps, DeviceBuffer) else maps.numel() * maps.element_size()
            nf, rem = divmod(nbytes, self.map_frame_bytes())
            if rem:
                raise ValueError(f"maps of {nbytes} B are not a whole number of frames ({self.map_frame_bytes()} B each)")
            cap = max(nf * 4096, 64) if det_cap is None else det_cap
            dn = DeviceBuffer(4 * L.STATUS_WORDS, self.device)
            own.append(dn)
            for _ in range(2):
                dd = DeviceBuffer(max(cap, 1) * DET_DTYPE.itemsize, self.device)
                try:
                    self.enqueue(maps, nf, dd, cap, dn)
                    # fmcw_memcpy is synchronous on the default stream the call ran on
                    found = int(dn.download(np.uint32, (L.STATUS_WORDS,))[0])
                    if found <= cap:
                        return dd.download(DET_DTYPE, (found,))
                finally:
                    dd.free()
                cap = found
            raise RuntimeError("detection count changed between two runs on the same maps")
        finally:
            for b in own:
                b.free()

    def set_grid_for_test(self, grid: int) -> None:
        """fmcw_cacfar_set_grid_for_test: at most `grid` workgroups for the two passes (0: the built-in
        bound), so that a small call drives a workgroup through several tiles and frames."""
        L.check(self._lib.fmcw_cacfar_set_grid_for_test(self._h, int(grid)))

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._lib.fmcw_cacfar_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
