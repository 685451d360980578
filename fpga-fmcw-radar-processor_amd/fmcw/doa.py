"""Angle resolution per detection (ctypes over fmcw_doa_*, include/fmcw.h).

``BearingEstimator`` reads one plane wave on a uniform line array: two targets in one range-Doppler cell
give it one blended bearing.  ``AngleResolver`` takes the channel snapshots that estimator writes and a
steering table ``A[g][k]`` (one row per grid point, geometry and calibration folded in) and gives, per
record, up to four sources: the strongest grid point of the scan ``|A[g]^H r|^2 / |A[g]|^2``, cancelled,
the next one, and so on, then ``relax_passes`` RELAX passes that re-estimate each source against the
others.  ``pos`` is the grid index refined by a three-point parabola (``refine``); ``line_steering``
returns the axis that turns it into ``sin_theta``.  The reference has one receive channel and no such
stage.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from ._object import DeviceObject, ptr, stage
from .radar_core import DeviceBuffer

DOA_DTYPE = np.dtype([("frame", "<u4"), ("range", "<u2"), ("doppler", "<u2"), ("flags", "<u4"), ("n_src", "<u4"),
                      ("total", "<f4"), ("residual", "<f4"), ("reserved", "<u4", (2,)),
                      ("src", [("grid", "<u4"), ("pos", "<f4"), ("amp_re", "<f4"), ("amp_im", "<f4")], (4,))])
assert DOA_DTYPE.itemsize == C.sizeof(L.FmcwDoa) == 96


def line_steering(n_ch: int, spacing: float, n_grid: int):
    """A uniform line array, element k at k * spacing wavelengths, on a grid uniform in sin_theta:
    (A complex64 [n_grid][n_ch], sin_theta float64 [n_grid]) with sin_theta[g] = -1 + 2 g / n_grid and
    A[g][k] = exp(2 pi i k spacing sin_theta[g]).  A source at position ``pos`` lies at
    sin_theta = -1 + 2 pos / n_grid, at nu = spacing * sin_theta cycles per element."""
    st = -1.0 + 2.0 * np.arange(n_grid) / n_grid
    a = np.exp(2j * np.pi * spacing * st[:, None] * np.arange(n_ch)[None, :])
    return a.astype(np.complex64), st


def planar_steering(positions_wavelengths, directions):
    """Any array: positions [n_ch][2 or 3] in wavelengths, directions [n_grid][2 or 3] direction cosines
    (u, v[, w]).  A[g][k] = exp(2 pi i positions[k] . directions[g]), complex64 [n_grid][n_ch].  The grid
    order is the caller's: use refine=False unless neighbouring rows are neighbouring angles."""
    p = np.asarray(positions_wavelengths, np.float64)
    u = np.asarray(directions, np.float64)
    if p.ndim != 2 or u.ndim != 2 or p.shape[1] != u.shape[1]:
        raise ValueError(f"positions {p.shape} and directions {u.shape} must be [n][2] or [n][3] alike")
    return np.exp(2j * np.pi * (u @ p.T)).astype(np.complex64)


def calibrated(steering, channel_gains):
    """The table of an array whose channel k measures channel_gains[k] (complex) times the ideal response."""
    a = np.asarray(steering)
    gk = np.asarray(channel_gains, np.complex128)
    if gk.shape != (a.shape[1],):
        raise ValueError(f"{gk.shape} gains for {a.shape[1]} channels")
    return (a * gk[None, :]).astype(np.complex64)


class AngleResolver(DeviceObject):
    _SYM = "fmcw_doa"

    def __init__(self, N_CH: int, steering, k_max: int = 2, relax_passes: int = 2, min_rel: float = 0.02,
                 refine: bool = True, max_records: int = 1 << 20, device: int = 0, n_grid: int | None = None):
        """steering: complex [n_grid][N_CH] (n_grid a multiple of 64, 64..1024), or None to set it later
        with set_steering / set_steering_dev (the table then has n_grid rows, 256 by default); until then no
        record has a source."""
        cfg = self._default_config(L.FmcwDoaConfig)
        st = None if steering is None else np.ascontiguousarray(steering, np.complex64)
        if st is not None and (st.ndim != 2 or st.shape[1] != N_CH):
            raise ValueError(f"steering {st.shape}: must be [n_grid][{N_CH}]")
        cfg.n_ch, cfg.k_max, cfg.relax_passes, cfg.min_rel = N_CH, k_max, relax_passes, min_rel
        if st is not None:
            cfg.n_grid = st.shape[0]
        elif n_grid is not None:
            cfg.n_grid = n_grid
        cfg.refine, cfg.max_records, cfg.device_id = int(refine), max_records, device
        self._create(cfg)
        if st is not None:
            self.set_steering(st)

    def set_steering(self, steering, stream: int = 0) -> None:
        """fmcw_doa_set_steering: a host table complex [n_grid][n_ch]; a row of norm 0 is an FmcwError."""
        st = np.ascontiguousarray(steering, np.complex64)
        if st.shape != (self.cfg.n_grid, self.cfg.n_ch):
            raise ValueError(f"steering {st.shape}: must be ({self.cfg.n_grid}, {self.cfg.n_ch})")
        L.check(self._lib.fmcw_doa_set_steering(self._h, st.ctypes.data, stream or None))

    def set_steering_dev(self, steering, stream: int = 0) -> None:
        """fmcw_doa_set_steering_dev: the same table in device memory, stream-ordered."""
        L.check(self._lib.fmcw_doa_set_steering_dev(self._h, ptr(steering), stream or None))

    def enqueue(self, snaps, cells, cell_stride: int, rec_cap: int, n_records, doa, spectrum, n_out, stream: int = 0):
        """Asynchronous, device pointers only (DeviceBuffer / torch CUDA tensors / ints).  snaps: complex64
        [record][n_ch], BearingEstimator.enqueue's; cells: None, or rec_cap records of cell_stride (16 or
        32) bytes that begin with frame / range / doppler (the BEARING_DTYPE records); n_records: their
        device count word; doa: room for min(rec_cap, max_records) records of DOA_DTYPE; spectrum: float32
        [record][n_grid] or None; n_out: 2 uint32 device words: records processed, without a snapshot."""
        L.check(self._lib.fmcw_doa_enqueue(self._h, ptr(snaps), ptr(cells), cell_stride, rec_cap, ptr(n_records),
                                           ptr(doa), ptr(spectrum), ptr(n_out), stream or None))

    def resolve(self, snaps, cells=None, want_spectrum: bool = False):
        """Synchronous.  snaps: a host complex64 array [record][n_ch]; cells: None or a host structured
        array of 16- or 32-byte records (BEARING_DTYPE, DET_DTYPE, PLOT_DTYPE), one per snapshot.
        Returns (DOA_DTYPE array, float32 [record][n_grid] spectrum or None)."""
        c = self.cfg
        sn = np.ascontiguousarray(snaps, np.complex64)
        if sn.ndim != 2 or sn.shape[1] != c.n_ch:
            raise ValueError(f"snaps {sn.shape}: must be [record][{c.n_ch}]")
        n = len(sn)
        if n > c.max_records:
            raise ValueError(f"{n} records exceed this resolver's max_records {c.max_records}")
        stride = 0
        if cells is not None:
            cells = np.ascontiguousarray(cells)
            stride = cells.dtype.itemsize
            if stride not in (16, 32) or len(cells) != n:
                raise TypeError(f"cells: {len(cells)} records of {stride} bytes for {n} snapshots (16 or 32 bytes each)")
        own = []
        try:
            ds, _ = stage(sn, np.complex64, 8, self.device, own)
            dc = None
            if cells is not None:
                dc = DeviceBuffer(max(n, 1) * stride, self.device)
                own.append(dc)
                if n:
                    dc.upload(cells)
            dn = DeviceBuffer(4, self.device)
            do = DeviceBuffer(max(n, 1) * DOA_DTYPE.itemsize, self.device)
            dsp = DeviceBuffer(max(n, 1) * c.n_grid * 4, self.device) if want_spectrum else None
            dst = DeviceBuffer(4 * L.DOA_STATUS_WORDS, self.device)
            own += [b for b in (dn, do, dsp, dst) if b is not None]
            dn.upload(np.array([n], np.uint32))
            self.enqueue(ds, dc, stride, n, dn, do, dsp, dst)
            # fmcw_memcpy is synchronous on the default stream the call ran on
            st = dst.download(np.uint32, (L.DOA_STATUS_WORDS,))
            assert int(st[0]) == n, st
            return do.download(DOA_DTYPE, (n,)), (dsp.download(np.float32, (n, c.n_grid)) if want_spectrum else None)
        finally:
            for b in own:
                b.free()

    def set_grid_for_test(self, grid: int) -> None:
        """fmcw_doa_set_grid_for_test: at most `grid` workgroups (0: the built-in bound), so that a short
        list drives a workgroup through several records."""
        super().set_grid_for_test(grid)
