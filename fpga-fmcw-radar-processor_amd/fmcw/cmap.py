"""Clutter-map detector: a threshold per cell from the cell's own history (ctypes over fmcw_cmap_*,
include/fmcw.h "Clutter map").

Every other detector here takes its threshold from a cell's neighbours within one frame, which goes wrong
at a clutter edge and in range-dependent clutter.  ``ClutterMap`` keeps, per stream (beam or sensor), an
exponential average of every cell over the scans, on the device and between calls, and detects a cell
that exceeds ``alpha`` times the largest average in its small neighbourhood.  It takes the maps
``RadarCore`` (``cfar="none"``) or ``BeamFormer`` write and gives the same ``DET_DTYPE`` list and status
words as ``RadarCore.cfar`` and ``CaCfar``, so ``PlotExtractor``, ``BearingEstimator`` and the device
tracker take its output unchanged.  The recurrence, the roundings and the order of the list are specified
in include/fmcw.h.
"""
from __future__ import annotations

import numpy as np

from . import _lib as L
from ._object import DeviceObject, detect_maps, ptr
from .radar_core import DeviceBuffer


class ClutterMap(DeviceObject):
    _SYM = "fmcw_cmap"

    def __init__(self, N_RANGE: int = 1024, N_DOPPLER: int = 128, n_streams: int = 1, gain: float = 0.125,
                 alpha: float = 4.0, floor: float = 0.0, clip: float = 0.0, spread=(1, 1), warmup: int = 8,
                 max_frames: int = 1, device: int = 0):
        """n_streams: independent maps; frame f of a call belongs to stream f % n_streams.  gain: the
        weight of a new scan in the average.  floor: the least threshold.  clip: 0, or the most a cell's
        input may exceed its average by (a factor) when it enters the average.  spread: (range, doppler)
        half extents, 0..4, of the neighbourhood whose largest average sets the threshold.  warmup: scans
        a stream must have seen before it detects."""
        cfg = self._default_config(L.FmcwCmapConfig)
        cfg.n_range, cfg.n_doppler, cfg.n_streams = N_RANGE, N_DOPPLER, n_streams
        cfg.gain, cfg.alpha, cfg.floor, cfg.clip = gain, alpha, floor, clip
        cfg.spread_range, cfg.spread_doppler = spread
        cfg.warmup, cfg.max_frames, cfg.device_id = warmup, max_frames, device
        self._create(cfg)

    def map_frame_bytes(self) -> int:
        return self.cfg.n_range * self.cfg.n_doppler * 4

    def state_bytes(self) -> tuple[int, int]:
        """(bytes of the planes, bytes of the ages) that get_state / set_state move."""
        return self.cfg.n_streams * self.map_frame_bytes(), self.cfg.n_streams * 4

    def enqueue(self, maps, n_frames: int, dets, det_cap: int, n_dets, stream: int = 0):
        """Asynchronous, device pointers only (DeviceBuffer / torch CUDA tensors / ints).  maps: n_frames
        float32 maps, n_frames a multiple of n_streams; dets: room for det_cap records (None with det_cap
        0); n_dets: FMCW_STATUS_WORDS (4) uint32 device words, [0] = detections found (may exceed
        det_cap).  The state advances by n_frames / n_streams scans whatever det_cap is."""
        L.check(self._lib.fmcw_cmap_enqueue(self._h, ptr(maps), n_frames, ptr(dets), det_cap, ptr(n_dets),
                                            stream or None))

    def reset(self, stream: int = 0) -> None:
        """Every stream's age goes to 0, in stream order: the next scan initialises the map."""
        L.check(self._lib.fmcw_cmap_reset(self._h, stream or None))

    def get_state(self, planes=None, ages=None, stream: int = 0):
        """With device pointers: a stream-ordered copy of the n_streams planes and / or age words into
        them.  With neither: synchronous, returns (planes float32 [stream][range][doppler], ages uint32)."""
        if planes is not None or ages is not None:
            L.check(self._lib.fmcw_cmap_get_state(self._h, ptr(planes), ptr(ages), stream or None))
            return None
        pb, ab = self.state_bytes()
        dp, da = DeviceBuffer(pb, self.device), DeviceBuffer(max(ab, 16), self.device)
        try:
            L.check(self._lib.fmcw_cmap_get_state(self._h, dp.ptr, da.ptr, None))
            # fmcw_memcpy is synchronous on the default stream the copy ran on
            return (dp.download(np.float32, (self.cfg.n_streams, self.cfg.n_range, self.cfg.n_doppler)),
                    da.download(np.uint32, (self.cfg.n_streams,)))
        finally:
            dp.free()
            da.free()

    def set_state(self, planes, ages=None, stream: int = 0) -> None:
        """planes (and ages, or None to keep them): host arrays (synchronous) or device pointers
        (stream-ordered).  Planes hold finite values >= 0."""
        own = []
        try:
            if isinstance(planes, np.ndarray):
                host = np.ascontiguousarray(planes, np.float32)
                if host.nbytes != self.state_bytes()[0]:
                    raise ValueError(f"planes of {host.nbytes} B, expected {self.state_bytes()[0]} B")
                planes = DeviceBuffer(host.nbytes, self.device)
                own.append(planes)
                planes.upload(host)
            if isinstance(ages, np.ndarray):
                host = np.ascontiguousarray(ages, np.uint32)
                if host.nbytes != self.state_bytes()[1]:
                    raise ValueError(f"ages of {host.nbytes} B, expected {self.state_bytes()[1]} B")
                ages = DeviceBuffer(max(host.nbytes, 16), self.device)
                own.append(ages)
                ages.upload(host)
            L.check(self._lib.fmcw_cmap_set_state(self._h, ptr(planes), ptr(ages), stream or None))
            if own:
                own[0].download(np.uint8, (1,))   # synchronous: the copy is done before the staging buffers go
        finally:
            for b in own:
                b.free()

    def detect(self, maps, det_cap: int | None = None) -> np.ndarray:
        """Synchronous.  maps: a host float32 array [frame][range][doppler] (or one map), or a
        DeviceBuffer / CUDA tensor holding whole maps.  Returns the DET_DTYPE list and advances the state
        by the call's scans, once: a rerun would advance it twice, so the state is saved before the call
        and restored before the single rerun when the first capacity was short."""
        pb, ab = self.state_bytes()
        sp, sa = DeviceBuffer(pb, self.device), DeviceBuffer(max(ab, 16), self.device)
        try:
            self.get_state(sp, sa)
            return detect_maps(self, maps, det_cap,
                               "detection count changed between two runs on the same maps and state",
                               before_rerun=lambda: self.set_state(sp, sa))
        finally:
            sp.free()
            sa.free()

    def set_grid_for_test(self, grid: int) -> None:
        """fmcw_cmap_set_grid_for_test: at most `grid` workgroups for the two passes (0: the built-in
        bound), so that a small call drives a workgroup through several (stream, tile) units."""
        super().set_grid_for_test(grid)
