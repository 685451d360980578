"""Velocity unfolding across a PRF stagger, between the plot extraction (or the beam merge) and the
tracker (ctypes over fmcw_unfold_*, include/fmcw.h).

A staggered radar changes its PRF from scan to scan, and a fast target's Doppler bin with it: the
fighter of ``synth.sea_scenario`` sits at bin 5, 8 and 10 of 32 at 8, 9 and 10 kHz.  Each PRF alone
knows the velocity only up to a multiple of itself.  ``VelocityUnfolder`` takes the record list of
many scans, groups every K consecutive scans of a stream (one per PRF) into a dwell and, for every
record, tries each velocity its bin can stand for: a hypothesis is a hit in another scan of the
dwell when a record lies where that velocity folds to at that scan's PRF.  The hypothesis with the
most hits wins (then the slower one), a report needs ``m_of`` hits, and the earliest scan that sees
the target owns it.  One ``VPLOT_DTYPE`` record per target and dwell: ``frame`` is
``dwell * n_streams + stream``, ``v_fine`` the velocity in units of f0 / n_doppler, ``doppler`` the
same on an axis of ``out_unit`` fine units per bin that does not change from scan to scan, so
``DeviceTwsTracker`` takes the records at stride 32 as they are, one tracker scan per dwell.
"""
from __future__ import annotations

import ctypes as C
from fractions import Fraction
from math import gcd

import numpy as np

from . import _lib as L
from ._object import DeviceObject, ptr, run_list

VPLOT_DTYPE = np.dtype([("frame", "<u4"), ("range", "<u2"), ("doppler", "<u2"), ("mag", "<f4"),
                        ("v_fine", "<i4"), ("fold", "<i2"), ("n_hits", "u1"), ("hit_mask", "u1"),
                        ("sum_mag", "<f4"), ("pos", "<u2"), ("n_ties", "<u2"), ("src", "<u4")])
assert VPLOT_DTYPE.itemsize == C.sizeof(L.FmcwVplot) == 32


class VelocityUnfolder(DeviceObject):
    _SYM = "fmcw_unfold"

    def __init__(self, N_RANGE: int = 1024, N_DOPPLER: int = 128, prf_units=(8, 9, 10), prf_phase: int = 0,
                 step: int | None = None, zero_bin: int = 0, v_max: int | None = None, out_unit: int | None = None,
                 tol=(1, 1), m_of: int = 2, n_streams: int = 1, max_recs: int = 1 << 20,
                 max_frames: int | None = None, device: int = 0):
        """prf_units: PRF k is prf_units[k] * f0; step: scans from one dwell to the next (default K: dwells
        do not overlap); v_max in fine units (default 2 * N_DOPPLER * min(prf_units)); out_unit: fine units
        per output Doppler bin (default min(prf_units)); tol = (range, Doppler) hit tolerance in bins."""
        cfg = self._default_config(L.FmcwUnfoldConfig)
        units = [int(p) for p in prf_units]
        if len(units) > 8:
            raise ValueError(f"{len(units)} PRFs: the stagger holds 2..8")
        cfg.n_range, cfg.n_doppler, cfg.n_prf = N_RANGE, N_DOPPLER, len(units)
        for k in range(8):
            cfg.prf_units[k] = units[k] if k < len(units) else 0
        p_min = min(units) if units else 1
        cfg.prf_phase, cfg.step, cfg.zero_bin = prf_phase, len(units) if step is None else step, zero_bin
        cfg.v_max = 2 * N_DOPPLER * p_min if v_max is None else v_max
        cfg.out_unit = p_min if out_unit is None else out_unit
        cfg.tol_range, cfg.tol_doppler = tol
        cfg.m_of, cfg.n_streams, cfg.max_recs, cfg.device_id = m_of, n_streams, max_recs, device
        # the default 1024 frames rounded up to whole scans
        cfg.max_frames = -(-1024 // max(n_streams, 1)) * max(n_streams, 1) if max_frames is None else max_frames
        self._create(cfg)

    @classmethod
    def from_physical(cls, prf_hz, wavelength_m: float, v_max_mps: float, n_doppler: int, **kw):
        """An unfolder for PRFs in Hz: f0 is their exact rational greatest common divisor (8, 9 and
        10 kHz: 1 kHz, units 8 / 9 / 10), v_max the largest radial speed in m/s.  Raises ValueError if no
        f0 gives units of at most 4096.  The result carries f0_hz and wavelength_m for velocity_mps."""
        fr = [Fraction(p).limit_denominator(1 << 20) for p in prf_hz]
        if not fr or any(f <= 0 for f in fr):
            raise ValueError("prf_hz: positive PRFs expected")
        den = 1
        for f in fr:
            den = den * f.denominator // gcd(den, f.denominator)
        num = 0
        for f in fr:
            num = gcd(num, int(f * den))
        f0 = Fraction(num, den)
        units = [int(f / f0) for f in fr]
        if max(units) > 4096:
            raise ValueError(f"PRFs {list(prf_hz)} Hz: their common divisor {float(f0)} Hz gives units up to {max(units)} (> 4096)")
        v_max = int(2.0 * v_max_mps / wavelength_m / (float(f0) / n_doppler))
        u = cls(N_DOPPLER=n_doppler, prf_units=units, v_max=v_max, **kw)
        u.f0_hz, u.wavelength_m = float(f0), float(wavelength_m)
        return u

    def enqueue(self, recs, rec_stride: int, rec_cap: int, n_recs, n_scans: int, out, out_cap: int, status,
                stream: int = 0):
        """Asynchronous, device pointers only (DeviceBuffer / torch CUDA tensors / ints).  recs: records
        of rec_stride 16 (fmcw_det) or 32 (fmcw_plot, fmcw_mplot) and n_recs their count word, as a
        detector, fmcw_plots_enqueue or fmcw_merge_enqueue wrote them; n_scans scans of n_streams
        frames each; status: FMCW_UNFOLD_STATUS_WORDS (4) uint32 device words: reports found (may exceed
        out_cap), records not examined, records at or beyond frame n_scans * n_streams (ignored),
        reports with more than one best hypothesis."""
        L.check(self._lib.fmcw_unfold_enqueue(self._h, ptr(recs), rec_stride, rec_cap, ptr(n_recs), n_scans,
                                              ptr(out), out_cap, ptr(status), stream or None))

    def unfold(self, records: np.ndarray, n_scans: int, out_cap: int | None = None) -> np.ndarray:
        """Synchronous: a host DET_DTYPE, PLOT_DTYPE or MPLOT_DTYPE array (sorted by frame, range,
        doppler; frame = scan * n_streams + stream) -> host VPLOT_DTYPE records; self.status holds the
        status words.  Reruns once with the reported count when out_cap was short."""
        r = np.ascontiguousarray(records)
        stride = r.dtype.itemsize
        if stride not in (16, 32):
            raise ValueError(f"records of {stride} B: DET_DTYPE (16) or PLOT_DTYPE (32) expected")
        n = len(r)
        if n > self.cfg.max_recs:
            raise ValueError(f"{n} records exceed this unfolder's max_recs {self.cfg.max_recs}")
        cap = max(n // 4, 64) if out_cap is None else out_cap
        out, self.status = run_list(self, r, 1, L.UNFOLD_STATUS_WORDS, VPLOT_DTYPE, cap,
                                    lambda dr, n, dn, do, cap, ds: self.enqueue(dr, stride, n, dn, n_scans, do, cap, ds),
                                    "report count changed between two runs on the same list")
        return out

    def n_dwells(self, n_scans: int) -> int:
        k, step = self.cfg.n_prf, self.cfg.step
        return (n_scans - k) // step + 1 if n_scans >= k else 0

    def set_grid_for_test(self, grid: int) -> None:
        """fmcw_unfold_set_grid_for_test: at most `grid` workgroups for the tile kernels (0: the
        built-in bound), so that a short list drives a workgroup through several tiles."""
        super().set_grid_for_test(grid)


def velocity_mps(vplots: np.ndarray, f0_hz: float, n_doppler: int, wavelength_m: float) -> np.ndarray:
    """Radial velocity in m/s (fp64): v_fine * f0 / n_doppler is the Doppler shift in Hz, times
    wavelength / 2."""
    return vplots["v_fine"].astype(np.float64) * (f0_hz / n_doppler) * (wavelength_m / 2.0)
