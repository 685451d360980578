"""Beam merge between the per-beam plot extraction and the tracker (ctypes over fmcw_merge_*,
include/fmcw.h).

After ``BeamFormer`` the chain runs on n_frames * n_beams maps and a record's ``frame`` is
``scan * n_beams + beam``.  Neighbouring beams overlap, so a target between two beams (or one whose
sidelobes cross the threshold next door) is a plot, and then a firm track, in each of them.
``BeamMerger`` is the plot extractor's peak grouping with the beam as a third axis: a record is a peak
when no other record of its neighbourhood (``win`` = (beam, range, Doppler) half-widths; Doppler
circular, range clamped, the beam axis clamped or, with ``beam_wrap``, circular; same scan) is
larger, ties going to the first in list order.  One ``MPLOT_DTYPE`` record per peak: ``frame`` is the
scan, ``beam`` + ``d_beam`` the magnitude-weighted beam position.  ``DeviceTwsTracker`` (one stream)
and ``BearingEstimator`` take the records at stride 32 as they are.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from ._object import DeviceObject, ptr, run_list

MPLOT_DTYPE = np.dtype([("frame", "<u4"), ("range", "<u2"), ("doppler", "<u2"), ("mag", "<f4"),
                        ("beam", "<u2"), ("n_merged", "<u2"), ("sum_mag", "<f4"),
                        ("d_beam", "<f4"), ("d_range", "<f4"), ("d_doppler", "<f4")])
assert MPLOT_DTYPE.itemsize == C.sizeof(L.FmcwMplot) == 32


class BeamMerger(DeviceObject):
    _SYM = "fmcw_merge"

    def __init__(self, N_RANGE: int = 1024, N_DOPPLER: int = 128, n_beams: int = 1, win=(1, 1, 1),
                 beam_wrap: bool = False, max_recs: int = 1 << 20, max_maps: int | None = None, device: int = 0):
        cfg = self._default_config(L.FmcwMergeConfig)
        cfg.n_range, cfg.n_doppler, cfg.n_beams = N_RANGE, N_DOPPLER, n_beams
        cfg.win_beam, cfg.win_range, cfg.win_doppler = win
        cfg.beam_wrap = int(beam_wrap)
        cfg.max_recs, cfg.device_id = max_recs, device
        # the default 1024 maps rounded up to whole scans
        cfg.max_maps = -(-1024 // max(n_beams, 1)) * max(n_beams, 1) if max_maps is None else max_maps
        self._create(cfg)

    def enqueue(self, recs, rec_stride: int, rec_cap: int, n_recs, n_maps: int, out, out_cap: int, status,
                stream: int = 0):
        """Asynchronous, device pointers only (DeviceBuffer / torch CUDA tensors / ints).  recs: records
        of rec_stride 16 (fmcw_det) or 32 (fmcw_plot) and n_recs their count word, as a detector or
        fmcw_plots_enqueue wrote them; n_maps = scans * n_beams; status: FMCW_MERGE_STATUS_WORDS (3)
        uint32 device words: merged plots found (may exceed out_cap), records not examined, records at
        or beyond frame n_maps (ignored)."""
        L.check(self._lib.fmcw_merge_enqueue(self._h, ptr(recs), rec_stride, rec_cap, ptr(n_recs), n_maps,
                                             ptr(out), out_cap, ptr(status), stream or None))

    def merge(self, records: np.ndarray, n_maps: int, out_cap: int | None = None) -> np.ndarray:
        """Synchronous: a host DET_DTYPE or PLOT_DTYPE array (sorted by frame, range, doppler; frame =
        scan * n_beams + beam) -> host MPLOT_DTYPE records.  Reruns once with the reported count when
        out_cap was short."""
        r = np.ascontiguousarray(records)
        stride = r.dtype.itemsize
        if stride not in (16, 32):
            raise ValueError(f"records of {stride} B: DET_DTYPE (16) or PLOT_DTYPE (32) expected")
        n = len(r)
        if n > self.cfg.max_recs:
            raise ValueError(f"{n} records exceed this merger's max_recs {self.cfg.max_recs}")
        cap = max(n // 4, 64) if out_cap is None else out_cap
        return run_list(self, r, 1, L.MERGE_STATUS_WORDS, MPLOT_DTYPE, cap,
                        lambda dr, n, dn, do, cap, ds: self.enqueue(dr, stride, n, dn, n_maps, do, cap, ds),
                        "merged-plot count changed between two runs on the same list")[0]

    def beam_position(self, mplots: np.ndarray) -> np.ndarray:
        """beam + d_beam in beams (fp64); with beam_wrap taken modulo n_beams."""
        return beam_position(mplots, self.cfg.n_beams, bool(self.cfg.beam_wrap))

    def interp(self, mplots: np.ndarray, per_beam_values, period: float | None = None) -> np.ndarray:
        """A per-beam table (each beam's sin(theta), say) at the merged plots' beam positions."""
        return interp(mplots, per_beam_values, bool(self.cfg.beam_wrap), period)

    def set_grid_for_test(self, grid: int) -> None:
        """fmcw_merge_set_grid_for_test: at most `grid` workgroups for the tile kernels (0: the
        built-in bound), so that a short list drives a workgroup through several tiles."""
        super().set_grid_for_test(grid)


def beam_position(mplots: np.ndarray, n_beams: int, beam_wrap: bool = False) -> np.ndarray:
    pos = mplots["beam"].astype(np.float64) + mplots["d_beam"].astype(np.float64)
    return np.mod(pos, n_beams) if beam_wrap else pos


def interp(mplots: np.ndarray, per_beam_values, beam_wrap: bool = False, period: float | None = None) -> np.ndarray:
    """Linear interpolation of per_beam_values (one value per beam) at beam + d_beam.  Without wrap the
    position is held inside [0, n_beams - 1].  With wrap the table is circular: between the last beam
    and beam 0 the value runs on to values[0] (+ or - `period`, when given, whichever is nearer: DFT
    beams' sin(theta) axis has period 2 / (2 spacing))."""
    v = np.asarray(per_beam_values, np.float64)
    nb = len(v)
    pos = beam_position(mplots, nb, beam_wrap)
    if not beam_wrap:
        return np.interp(pos, np.arange(nb), v)
    i0 = np.floor(pos).astype(np.int64) % nb
    t = pos - np.floor(pos)
    v0, v1 = v[i0], v[(i0 + 1) % nb]
    if period:
        v1 = v0 + np.mod(v1 - v0 + period / 2, period) - period / 2
    return v0 + t * (v1 - v0)
