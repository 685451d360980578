"""Track-while-scan tracker on the device (ctypes over fmcw_tws_dev_*, include/fmcw.h).

``TwsTracker`` (fmcw.tracker) is host code fed one frame at a time.  ``DeviceTwsTracker`` runs the
same tracker -- the same generics, the same integers, both ``rtl_compat`` values -- over a record
list that is already on the device, as fmcw_enqueue / fmcw_cfar / the cell-averaging detector / the
plot extractor wrote it: many scans per call, ``n_streams`` independent track files side by side
(record frame ``m`` is scan ``m // n_streams`` of stream ``m % n_streams``, the beamformer's
``f * n_beams + b``), stream-ordered and capturable into a graph.  The track files live on the
device and persist from call to call, so a replayed graph advances them; ``reset`` puts them back.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from ._object import DeviceObject, ptr
from .plots import PLOT_DTYPE
from .radar_core import DET_DTYPE, DeviceBuffer
from .tracker import TRACK_DTYPE

assert TRACK_DTYPE.itemsize == C.sizeof(L.FmcwTrack) == 28


class DeviceTwsTracker(DeviceObject):
    _SYM = "fmcw_tws_dev"

    def __init__(self, n_streams: int = 1, max_scans: int = 1024, device: int = 0, MAX_TRACKS: int = 32,
                 INIT_HITS: int = 2, COAST_MAX: int = 5, ASSOC_GATE_R: int = 10, ASSOC_GATE_D: int = 5,
                 ALPHA_GAIN: int = 128, BETA_GAIN: int = 64, MAX_DETS: int = 64, rtl_compat: bool = False):
        cfg = self._default_config(L.FmcwTwsDevConfig)
        t = cfg.tws
        t.max_tracks, t.max_dets, t.init_hits, t.coast_max = MAX_TRACKS, MAX_DETS, INIT_HITS, COAST_MAX
        t.gate_r, t.gate_d, t.alpha_q8, t.beta_q8 = ASSOC_GATE_R, ASSOC_GATE_D, ALPHA_GAIN, BETA_GAIN
        t.rtl_compat = int(bool(rtl_compat))
        cfg.n_streams, cfg.max_scans, cfg.device_id = n_streams, max_scans, device
        self._create(cfg)

    def enqueue(self, recs, rec_stride: int, rec_cap: int, n_recs, n_scans: int, tracks, track_cap: int,
                counts, status, stream: int = 0):
        """Asynchronous, device pointers only (DeviceBuffer / torch CUDA tensors / ints).  recs and
        n_recs as the producer wrote them (rec_stride 16: fmcw_det, 32: fmcw_plot); tracks:
        n_scans x n_streams x track_cap TRACK_DTYPE records; counts: 2 words per (scan, stream)
        (tracks reported, active tracks); status: FMCW_TWS_DEV_STATUS_WORDS (2) words (records not
        examined, examined records at or beyond frame n_scans x n_streams)."""
        L.check(self._lib.fmcw_tws_dev_enqueue(self._h, ptr(recs), rec_stride, rec_cap, ptr(n_recs), n_scans,
                                               ptr(tracks), track_cap, ptr(counts), ptr(status),
                                               stream or None))

    def run(self, records: np.ndarray, n_scans: int):
        """Synchronous: a host DET_DTYPE or PLOT_DTYPE array with non-decreasing frames -> a list over
        scans of lists over streams of (TRACK_DTYPE array, active_tracks)."""
        r = np.asarray(records)
        if r.dtype not in (DET_DTYPE, PLOT_DTYPE):
            r = np.ascontiguousarray(r, dtype=DET_DTYPE)
        r = np.ascontiguousarray(r)
        n, ns, cap = len(r), self.cfg.n_streams, self.cfg.tws.max_tracks
        groups = n_scans * ns
        dr = DeviceBuffer(max(r.nbytes, 4), self.device)
        dn = DeviceBuffer(4 * L.STATUS_WORDS, self.device)
        dt = DeviceBuffer(max(groups, 1) * cap * TRACK_DTYPE.itemsize, self.device)
        dc = DeviceBuffer(max(groups, 1) * 8, self.device)
        ds = DeviceBuffer(4 * L.TWS_DEV_STATUS_WORDS, self.device)
        try:
            if n:
                dr.upload(r)
            dn.upload(np.array([n, 0, 0, 0], np.uint32))
            self.enqueue(dr, r.dtype.itemsize, n, dn, n_scans, dt, cap, dc, ds)
            # fmcw_memcpy is synchronous on the default stream the call ran on
            self.status = ds.download(np.uint32, (L.TWS_DEV_STATUS_WORDS,))
            if not groups:
                return []
            counts = dc.download(np.uint32, (groups, 2))
            tracks = dt.download(TRACK_DTYPE, (groups, cap))
        finally:
            for b in (dr, dn, dt, dc, ds):
                b.free()
        return [[(tracks[m, :counts[m, 0]].copy(), int(counts[m, 1])) for m in range(s * ns, (s + 1) * ns)]
                for s in range(n_scans)]

    def reset(self, stream: int = 0) -> None:
        """fmcw_tws_dev_reset: every track file back to power-up, in stream order."""
        L.check(self._lib.fmcw_tws_dev_reset(self._h, stream or None))

    def set_grid_for_test(self, grid: int) -> None:
        """fmcw_tws_dev_set_grid_for_test: at most `grid` workgroups for both kernels (0: the built-in
        bound), so that a short list drives the index kernel through several tiles and one wave of
        the tracker through several streams."""
        super().set_grid_for_test(grid)
