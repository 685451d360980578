"""Coherent beamforming (ctypes over fmcw_beams_*, include/fmcw.h).

With ``N_RX > 1`` RadarCore's map is the non-coherent sum over the channels: about sqrt(N_RX) in SNR.
``BeamFormer`` takes the corner-turned spectrum of ``RadarCore.range_ct`` and a complex weight matrix
``[beam][rx]`` and gives one range-Doppler magnitude map per (frame, beam): the channels are weighted
and summed before the Doppler transform, so a beam steered at a target gains N_RX, and two targets in
one range-Doppler cell separate in angle.  The maps are laid out ``[frame][beam][range][doppler]``,
so ``RadarCore.cfar`` runs on them as ``n_frames * n_beams`` frames; a detection's ``frame`` is then
``f * n_beams + b``.  The reference is a single-channel core and has no such stage.
"""
from __future__ import annotations

import numpy as np

from . import _lib as L
from ._object import DeviceObject, ptr, stage
from .radar_core import DeviceBuffer

_WINDOWS = {"hamming": L.WIN_HAMMING, "none": L.WIN_NONE}
_MTI = {0: L.MTI_OFF, 2: L.MTI_2PULSE, 3: L.MTI_3PULSE}


def steering_weights(n_rx: int, nus, taper=None) -> np.ndarray:
    """complex64 [beam][rx] for a uniform line array: W[b][k] = t_k exp(-2 pi i nus[b] k) / sum_k t_k,
    unit gain for a plane wave at nus[b] cycles per element (the sign of synth's rx_phase and of the
    bearing estimator's nu).  taper: n_rx real amplitudes t_k (default all ones)."""
    nus = np.atleast_1d(np.asarray(nus, np.float64))
    t = np.ones(n_rx) if taper is None else np.asarray(taper, np.float64)
    if nus.ndim != 1 or t.shape != (n_rx,):
        raise ValueError(f"nus must be a list of beams and taper must have n_rx = {n_rx} entries")
    if not t.sum() > 0:
        raise ValueError("taper must have a positive sum")
    k = np.arange(n_rx)
    return (t * np.exp(-2j * np.pi * nus[:, None] * k[None, :]) / t.sum()).astype(np.complex64)


class BeamFormer(DeviceObject):
    _SYM = "fmcw_beams"

    def __init__(self, N_RANGE: int, N_DOPPLER: int, N_RX: int, weights, window: str = "hamming", mti: int = 0,
                 device: int = 0):
        """weights: complex [beam][rx] (steering_weights, or any matrix: taper and channel calibration
        are the caller's).  window: "hamming" or "none"; mti: 0 (off), 2 or 3 (pulse canceller)."""
        w = np.ascontiguousarray(weights, dtype=np.complex64)
        if w.ndim != 2 or w.shape[1] != N_RX:
            raise ValueError(f"weights must be [beam][rx] with rx = {N_RX}, not {w.shape}")
        cfg = self._default_config(L.FmcwBeamsConfig)
        cfg.n_range, cfg.n_doppler, cfg.n_rx, cfg.n_beams = N_RANGE, N_DOPPLER, N_RX, w.shape[0]
        cfg.window = _WINDOWS[window] if isinstance(window, str) else window
        cfg.mti_mode = _MTI.get(mti, mti)
        cfg.device_id = device
        self.weights = w
        self._create(cfg, w.ctypes.data)

    @property
    def n_beams(self) -> int:
        return self.cfg.n_beams

    def spec_frame_bytes(self) -> int:
        c = self.cfg
        return c.n_rx * c.n_range * c.n_doppler * 8

    def maps_frame_bytes(self) -> int:
        c = self.cfg
        return c.n_beams * c.n_range * c.n_doppler * 4

    def enqueue(self, spec, n_frames: int, maps, stream: int = 0):
        """Asynchronous, device pointers only (DeviceBuffer / torch CUDA tensors / ints).  spec: n_frames
        frames of range_ct output; maps: room for n_frames * n_beams float32 maps, 16-byte aligned."""
        L.check(self._lib.fmcw_beams_enqueue(self._h, ptr(spec), n_frames, ptr(maps), stream or None))

    def set_weights_dev(self, w, stream: int = 0) -> None:
        """fmcw_beams_set_weights_dev: replace the matrix by n_beams x n_rx complex64 on the device
        (AdaptiveWeights.enqueue's w), stream-ordered and capturable.  Nothing checks the values:
        weights that are not finite give maps that are not finite.  `self.weights` keeps the matrix
        of the constructor."""
        L.check(self._lib.fmcw_beams_set_weights_dev(self._h, ptr(w), stream or None))

    def form(self, spec) -> np.ndarray:
        """Synchronous.  spec: range_ct output as a DeviceBuffer / CUDA tensor, or a host complex64
        array [frame][rx][range][chirp].  Returns float32 [frame][beam][range][doppler]."""
        c = self.cfg
        own = []
        try:
            spec, nbytes = stage(spec, np.complex64, 8, self.device, own)
            nf, rem = divmod(nbytes, self.spec_frame_bytes())
            if rem:
                raise ValueError(f"spectrum of {nbytes} B is not a whole number of frames "
                                 f"({self.spec_frame_bytes()} B each)")
            dm = DeviceBuffer(max(nf * self.maps_frame_bytes(), 16), self.device)
            own.append(dm)
            self.enqueue(spec, nf, dm)
            # fmcw_memcpy is synchronous on the default stream the call ran on
            return dm.download(np.float32, (nf, c.n_beams, c.n_range, c.n_doppler))
        finally:
            for b in own:
                b.free()

    def set_grid_for_test(self, grid: int) -> None:
        """fmcw_beams_set_grid_for_test: at most `grid` workgroups (0: the built-in bound), so that a
        small call drives a workgroup through several tiles, frames and beams."""
        super().set_grid_for_test(grid)
