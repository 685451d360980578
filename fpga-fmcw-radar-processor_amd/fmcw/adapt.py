"""Adaptive beam weights (ctypes over fmcw_adapt_*, include/fmcw.h).

``BeamFormer`` applies the matrix it is given.  ``AdaptiveWeights`` computes one from the data: the
sample covariance R of the receive channels over a training window of ``RadarCore.range_ct``'s
spectrum, diagonally loaded, and the minimum-variance (MVDR) weights that hold each look direction
``a_b`` at unit gain:

    W[b] = conj(Rl^-1 a_b) / (a_b^H Rl^-1 a_b),   Rl = R + loading * tr(R) / n_rx * I

A strong off-axis emitter is nulled; with white noise alone W is the conventional beam.  The weights
stay on the device: ``enqueue`` then ``BeamFormer.set_weights_dev`` then ``BeamFormer.enqueue``, on one
stream, capturable into a graph.  The reference is a single-channel core and has no such stage.
"""
from __future__ import annotations

import numpy as np

from . import _lib as L
from ._object import DeviceObject, ptr, stage
from .radar_core import DeviceBuffer

_MTI = {0: L.MTI_OFF, 2: L.MTI_2PULSE, 3: L.MTI_3PULSE}
ADAPT_FALLBACK = 1       # FMCW_ADAPT_FALLBACK
INFO_WORDS = 8           # FMCW_ADAPT_INFO_WORDS


def steering_vectors(n_rx: int, nus) -> np.ndarray:
    """complex64 [beam][rx] array responses of a uniform line array, a_b[k] = exp(2 pi i nus[b] k):
    the look directions whose conventional weights are ``steering_weights(n_rx, nus)``."""
    nus = np.atleast_1d(np.asarray(nus, np.float64))
    if nus.ndim != 1:
        raise ValueError("nus must be a list of beams")
    return np.exp(2j * np.pi * nus[:, None] * np.arange(n_rx)[None, :]).astype(np.complex64)


def parse_info(words: np.ndarray) -> dict:
    """The status words of fmcw_adapt_enqueue: K, flags, n_units, delta (fp64) and fallback."""
    w = np.asarray(words, np.uint32)
    return {"K": int(w[0]) | int(w[1]) << 32, "flags": int(w[2]), "n_units": int(w[3]),
            "delta": float(w[4:6].copy().view(np.float64)[0]), "fallback": bool(int(w[2]) & ADAPT_FALLBACK)}


class AdaptiveWeights(DeviceObject):
    _SYM = "fmcw_adapt"

    def __init__(self, N_RANGE: int, N_DOPPLER: int, N_RX: int, constraints, loading: float = 1e-2, mti: int = 0,
                 train_r0: int = 0, train_rows: int | None = None, device: int = 0):
        """constraints: complex [beam][rx], the array response a_b of each look direction
        (steering_vectors).  Training rows [train_r0, train_r0 + train_rows) (default: the whole map)."""
        a = np.ascontiguousarray(constraints, dtype=np.complex64)
        if a.ndim != 2 or a.shape[1] != N_RX:
            raise ValueError(f"constraints must be [beam][rx] with rx = {N_RX}, not {a.shape}")
        cfg = self._default_config(L.FmcwAdaptConfig)
        cfg.n_range, cfg.n_doppler, cfg.n_rx, cfg.n_beams = N_RANGE, N_DOPPLER, N_RX, a.shape[0]
        cfg.mti_mode = _MTI.get(mti, mti)
        cfg.train_r0 = train_r0
        cfg.train_rows = N_RANGE - train_r0 if train_rows is None else train_rows
        cfg.loading = loading
        cfg.device_id = device
        self.constraints = a
        self._create(cfg, a.ctypes.data)

    @property
    def n_beams(self) -> int:
        return self.cfg.n_beams

    def spec_frame_bytes(self) -> int:
        c = self.cfg
        return c.n_rx * c.n_range * c.n_doppler * 8

    def w_bytes(self) -> int:
        return self.cfg.n_beams * self.cfg.n_rx * 8

    def cov_bytes(self) -> int:
        return self.cfg.n_rx * self.cfg.n_rx * 16

    def enqueue(self, spec, n_frames: int, w, cov, info, stream: int = 0):
        """Asynchronous, device pointers only (DeviceBuffer / torch CUDA tensors / ints).  spec: n_frames
        frames of range_ct output; w: n_beams x n_rx complex64; cov: n_rx x n_rx complex128 or None;
        info: 8 uint32 words (parse_info)."""
        L.check(self._lib.fmcw_adapt_enqueue(self._h, ptr(spec), n_frames, ptr(w), ptr(cov), ptr(info),
                                             stream or None))

    def solve(self, spec):
        """Synchronous.  spec: range_ct output as a DeviceBuffer / CUDA tensor, or a host complex64
        array [frame][rx][range][chirp].  Returns (W complex64 [beam][rx], R complex128 [rx][rx], info)."""
        c = self.cfg
        own = []
        try:
            spec, nbytes = stage(spec, np.complex64, 8, self.device, own)
            nf, rem = divmod(nbytes, self.spec_frame_bytes())
            if rem or nf == 0:
                raise ValueError(f"spectrum of {nbytes} B is not a whole, positive number of frames "
                                 f"({self.spec_frame_bytes()} B each)")
            dw, dr, di = (DeviceBuffer(n, self.device) for n in (self.w_bytes(), self.cov_bytes(), 4 * INFO_WORDS))
            own += [dw, dr, di]
            self.enqueue(spec, nf, dw, dr, di)
            # fmcw_memcpy is synchronous on the default stream the call ran on
            return (dw.download(np.complex64, (c.n_beams, c.n_rx)), dr.download(np.complex128, (c.n_rx, c.n_rx)),
                    parse_info(di.download(np.uint32, (INFO_WORDS,))))
        finally:
            for b in own:
                b.free()

    def set_grid_for_test(self, grid: int) -> None:
        """fmcw_adapt_set_grid_for_test: at most `grid` workgroups (0: the built-in bound), so that a
        small call drives a wave through several units."""
        super().set_grid_for_test(grid)
