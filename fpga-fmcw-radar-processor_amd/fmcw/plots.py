"""Plot extraction (peak grouping) between the CFAR and the tracker (ctypes over fmcw_plots_*,
include/fmcw.h).

The reference streams every CFAR output into tws_tracker, which keeps a scan's first 64
(rtl/src/tws_tracker.vhd MAX_DETS); a point target's Hamming main lobe and Doppler sidelobes are
dozens of detections, so the nearest target takes every slot.  ``PlotExtractor`` reduces the
detection list to one plot per local maximum on the device: a detection is a peak when no other
detection of its window (``win`` = (range, Doppler) half-widths, Doppler circular, range clamped,
same frame) is larger, ties going to the first in list order.  ``TwsTracker.scan`` accepts
``PLOT_DTYPE`` records as they are (it reads range / doppler / mag / frame by name).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from ._object import DeviceObject, ptr, run_list
from .radar_core import DET_DTYPE

PLOT_DTYPE = np.dtype([("frame", "<u4"), ("range", "<u2"), ("doppler", "<u2"), ("mag", "<f4"),
                       ("threshold", "<f4"), ("n_cells", "<u4"), ("sum_mag", "<f4"),
                       ("d_range", "<f4"), ("d_doppler", "<f4")])
assert PLOT_DTYPE.itemsize == C.sizeof(L.FmcwPlot) == 32


class PlotExtractor(DeviceObject):
    _SYM = "fmcw_plots"

    def __init__(self, N_RANGE: int = 1024, N_DOPPLER: int = 128, win=(1, 1), max_dets: int = 1 << 20,
                 device: int = 0):
        cfg = self._default_config(L.FmcwPlotsConfig)
        cfg.n_range, cfg.n_doppler = N_RANGE, N_DOPPLER
        cfg.win_range, cfg.win_doppler = win
        cfg.max_dets, cfg.device_id = max_dets, device
        self._create(cfg)

    def enqueue(self, dets, det_cap: int, n_dets, plots, plot_cap: int, n_plots, stream: int = 0):
        """Asynchronous, device pointers only (DeviceBuffer / torch CUDA tensors / ints).  dets and
        n_dets as fmcw_enqueue wrote them; n_plots: FMCW_PLOT_STATUS_WORDS (2) uint32 device words:
        plots found (may exceed plot_cap), records not examined."""
        L.check(self._lib.fmcw_plots_enqueue(self._h, ptr(dets), det_cap, ptr(n_dets), ptr(plots),
                                             plot_cap, ptr(n_plots), stream or None))

    def extract(self, dets: np.ndarray, plot_cap: int | None = None) -> np.ndarray:
        """Synchronous: a host DET_DTYPE array (sorted by frame, range, doppler) -> host PLOT_DTYPE
        plots.  Retries once with the reported count when plot_cap was short."""
        d = np.ascontiguousarray(dets, dtype=DET_DTYPE)
        n = len(d)
        if n > self.cfg.max_dets:
            raise ValueError(f"{n} detections exceed this extractor's max_dets {self.cfg.max_dets}")
        cap = max(n // 4, 64) if plot_cap is None else plot_cap
        return run_list(self, d, L.STATUS_WORDS, L.PLOT_STATUS_WORDS, PLOT_DTYPE, cap, self.enqueue,
                        "plot count changed between two runs on the same list")[0]

    def set_grid_for_test(self, grid: int) -> None:
        """fmcw_plots_set_grid_for_test: at most `grid` workgroups for the two tile kernels (0: the
        built-in bound), so that a short list drives a workgroup through several tiles."""
        super().set_grid_for_test(grid)
