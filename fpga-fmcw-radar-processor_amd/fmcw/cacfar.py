"""Cell-averaging CFAR: CA, greatest-of and smallest-of (ctypes over fmcw_cacfar_*, include/fmcw.h).

The reference's detectors are ordered-statistic (RadarCore's "os1d" / "os2d"), whose cost follows the
data.  ``CaCfar`` is the detector whose cost does not: the same sums on every cell of a range-Doppler
map, two reads of the map per call.  It takes the maps ``RadarCore`` (``cfar="none"``) or
``BeamFormer`` write, and gives the same ``DET_DTYPE`` list and status words as ``RadarCore.cfar``, so
``PlotExtractor``, ``BearingEstimator`` and the gather take its output unchanged.  The window, the
canonical order of the sums and the thresholds are specified in include/fmcw.h.
"""
from __future__ import annotations

import numpy as np

from . import _lib as L
from ._object import DeviceObject, detect_maps, ptr

_MODES = {"ca": L.CACFAR_CA, "go": L.CACFAR_GO, "so": L.CACFAR_SO}


class CaCfar(DeviceObject):
    _SYM = "fmcw_cacfar"

    def __init__(self, N_RANGE: int = 1024, N_DOPPLER: int = 128, mode: str = "ca", ref=(4, 4), guard=(1, 2),
                 alpha: float = 4.0, max_frames: int = 1, device: int = 0):
        """mode: "ca" (T = alpha x mean of the window), "go" / "so" (alpha x the larger / smaller of the
        two half-window means).  ref, guard: (range, doppler) extents, 0..8 and 0..4."""
        cfg = self._default_config(L.FmcwCaCfarConfig)
        cfg.n_range, cfg.n_doppler = N_RANGE, N_DOPPLER
        cfg.mode = _MODES[mode] if isinstance(mode, str) else mode
        cfg.ref_range, cfg.ref_doppler = ref
        cfg.guard_range, cfg.guard_doppler = guard
        cfg.alpha = alpha
        cfg.max_frames, cfg.device_id = max_frames, device
        self._create(cfg)

    def map_frame_bytes(self) -> int:
        return self.cfg.n_range * self.cfg.n_doppler * 4

    def enqueue(self, maps, n_frames: int, dets, det_cap: int, n_dets, stream: int = 0):
        """Asynchronous, device pointers only (DeviceBuffer / torch CUDA tensors / ints).  maps: n_frames
        float32 maps; dets: room for det_cap records (None with det_cap 0 counts only); n_dets:
        FMCW_STATUS_WORDS (4) uint32 device words, [0] = detections found (may exceed det_cap)."""
        L.check(self._lib.fmcw_cacfar_enqueue(self._h, ptr(maps), n_frames, ptr(dets), det_cap, ptr(n_dets),
                                              stream or None))

    def detect(self, maps, det_cap: int | None = None) -> np.ndarray:
        """Synchronous.  maps: a host float32 array [frame][range][doppler] (or one map), or a
        DeviceBuffer / CUDA tensor holding whole maps.  Returns the DET_DTYPE list; reruns once with the
        reported count when the first capacity was short."""
        return detect_maps(self, maps, det_cap, "detection count changed between two runs on the same maps")

    def set_grid_for_test(self, grid: int) -> None:
        """fmcw_cacfar_set_grid_for_test: at most `grid` workgroups for the two passes (0: the built-in
        bound), so that a small call drives a workgroup through several tiles and frames."""
        super().set_grid_for_test(grid)
