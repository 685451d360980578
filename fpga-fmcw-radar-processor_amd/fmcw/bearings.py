"""Bearing estimation per detection or plot (ctypes over fmcw_bearings_*, include/fmcw.h).

With ``N_RX > 1`` RadarCore's map is the non-coherent sum over the channels, and the phase across
them -- a target's angle -- is in no output of ``process`` / ``enqueue``.  ``BearingEstimator``
takes the corner-turned spectrum of ``RadarCore.range_ct`` and a record list (``DET_DTYPE`` or
``PLOT_DTYPE``) and gives, per record, the rx snapshot s_k (the cell's complex Doppler bin per
channel) and from it ``nu`` (phase step in cycles per element of a uniform line array),
``sin_theta = nu / spacing``, ``power`` (the NCI magnitude) and ``coherence`` (1 for one plane
wave).  The reference is a single-channel core and has no such stage.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from ._object import DeviceObject, ptr, stage
from .plots import PLOT_DTYPE
from .radar_core import DET_DTYPE, DeviceBuffer

BEARING_DTYPE = np.dtype([("frame", "<u4"), ("range", "<u2"), ("doppler", "<u2"), ("flags", "<u4"),
                          ("nu", "<f4"), ("sin_theta", "<f4"), ("power", "<f4"), ("coherence", "<f4"),
                          ("reserved", "<u4")])
assert BEARING_DTYPE.itemsize == C.sizeof(L.FmcwBearing) == 32

_WINDOWS = {"hamming": L.WIN_HAMMING, "none": L.WIN_NONE}
_MTI = {0: L.MTI_OFF, 2: L.MTI_2PULSE, 3: L.MTI_3PULSE}


class BearingEstimator(DeviceObject):
    _SYM = "fmcw_bearings"

    def __init__(self, N_RANGE: int = 1024, N_DOPPLER: int = 128, N_RX: int = 1, window: str = "hamming",
                 mti: int = 0, spacing: float = 0.5, max_records: int = 1 << 20, device: int = 0):
        """window: "hamming" or "none"; mti: 0 (off), 2 or 3 (pulse canceller) -- those of the
        RadarCore whose detections are located, so that ``power`` is the map's cell.  spacing: element
        spacing in wavelengths."""
        cfg = self._default_config(L.FmcwBearingsConfig)
        cfg.n_range, cfg.n_doppler, cfg.n_rx = N_RANGE, N_DOPPLER, N_RX
        cfg.window = _WINDOWS[window] if isinstance(window, str) else window
        cfg.mti_mode = _MTI.get(mti, mti)
        cfg.spacing, cfg.max_records, cfg.device_id = spacing, max_records, device
        self._create(cfg)

    def spec_frame_bytes(self) -> int:
        c = self.cfg
        return c.n_rx * c.n_range * c.n_doppler * 8

    def enqueue(self, spec, n_frames: int, records, rec_stride: int, rec_cap: int, n_records, bearings,
                snaps, n_out, stream: int = 0):
        """Asynchronous, device pointers only (DeviceBuffer / torch CUDA tensors / ints).  spec:
        n_frames frames of range_ct output; records: rec_cap records of rec_stride (16 or 32) bytes and
        n_records their device count word; bearings: room for min(rec_cap, max_records) records of
        BEARING_DTYPE; snaps: complex64 [record][rx] or None; n_out: FMCW_BEARING_STATUS_WORDS (2)
        uint32 device words: records processed, out-of-range records among them."""
        L.check(self._lib.fmcw_bearings_enqueue(self._h, ptr(spec), n_frames, ptr(records), rec_stride, rec_cap,
                                                ptr(n_records), ptr(bearings), ptr(snaps), ptr(n_out),
                                                stream or None))

    def estimate(self, spec, records: np.ndarray, want_snaps: bool = True):
        """Synchronous.  spec: range_ct output as a DeviceBuffer / CUDA tensor, or a host complex64
        array [frame][rx][range][chirp]; records: a host DET_DTYPE or PLOT_DTYPE array.  Returns
        (BEARING_DTYPE array, complex64 [record][rx] snapshots or None)."""
        rec = np.ascontiguousarray(records)
        if rec.dtype not in (DET_DTYPE, PLOT_DTYPE):
            raise TypeError(f"records must be DET_DTYPE or PLOT_DTYPE, not {rec.dtype}")
        n, stride = len(rec), rec.dtype.itemsize
        if n > self.cfg.max_records:
            raise ValueError(f"{n} records exceed this estimator's max_records {self.cfg.max_records}")
        own = []
        try:
            spec, nbytes = stage(spec, np.complex64, 8, self.device, own)
            nf, rem = divmod(nbytes, self.spec_frame_bytes())
            if rem:
                raise ValueError(f"spectrum of {nbytes} B is not a whole number of frames "
                                 f"({self.spec_frame_bytes()} B each)")
            nrx = self.cfg.n_rx
            dr = DeviceBuffer(max(n, 1) * stride, self.device)
            dn = DeviceBuffer(4, self.device)
            db = DeviceBuffer(max(n, 1) * BEARING_DTYPE.itemsize, self.device)
            ds = DeviceBuffer(max(n, 1) * nrx * 8, self.device) if want_snaps else None
            dst = DeviceBuffer(4 * L.BEARING_STATUS_WORDS, self.device)
            own += [b for b in (dr, dn, db, ds, dst) if b is not None]
            if n:
                dr.upload(rec)
            dn.upload(np.array([n], np.uint32))
            self.enqueue(spec, nf, dr, stride, n, dn, db, ds, dst)
            # fmcw_memcpy is synchronous on the default stream the call ran on
            st = dst.download(np.uint32, (L.BEARING_STATUS_WORDS,))
            assert int(st[0]) == n, st
            out = db.download(BEARING_DTYPE, (n,))
            snaps = ds.download(np.complex64, (n, nrx)) if want_snaps else None
            return out, snaps
        finally:
            for b in own:
                b.free()

    def set_grid_for_test(self, grid: int) -> None:
        """fmcw_bearings_set_grid_for_test: at most `grid` workgroups (0: the built-in bound), so that
        a short list drives a workgroup through several records."""
        super().set_grid_for_test(grid)
