"""The TDM-MIMO virtual array (ctypes over fmcw_mimo_*, include/fmcw.h).

A front end whose ``N_TX`` transmitters fire in turn, chirp by chirp, has ``N_TX * N_RX`` virtual channels.
``VirtualArray`` takes the corner-turned spectrum of ``RadarCore.range_ct`` for ``N_CHIRPS = N_TX * n_d``
chirps and gives a spectrum ``[frame][n_tx * n_rx][range][n_d]`` that ``BearingEstimator``, ``BeamFormer``
and ``AdaptiveWeights`` read unchanged as ``N_RX = n_virtual`` channels of ``N_DOPPLER = n_d`` chirps.
Channel ``t * N_RX + k`` is transmitter t (the chirps ``c = m * N_TX + t``) seen by receiver k.  With
``align="dft"`` transmitter t's sequence is delayed by ``t / N_TX`` samples, so that a moving target's
Doppler leaves no phase step between the TX blocks; ``align="none"`` is the raw de-interleave.  The
reference has one transmitter and no such stage.
"""
from __future__ import annotations

import numpy as np

from . import _lib as L
from ._object import DeviceObject, ptr, stage
from .radar_core import DeviceBuffer

_ALIGN = {"dft": L.MIMO_ALIGN_DFT, "none": L.MIMO_ALIGN_NONE}


class VirtualArray(DeviceObject):
    _SYM = "fmcw_mimo"

    def __init__(self, N_RANGE: int, N_CHIRPS: int, N_RX: int, N_TX: int, align: str = "dft", device: int = 0):
        """N_CHIRPS: the chirps of a frame, all transmitters together (range_ct's N_DOPPLER); N_TX: a power
        of two, transmitter t firing in slot t.  align: "dft" (time-aligned) or "none" (a copy)."""
        cfg = self._default_config(L.FmcwMimoConfig)
        cfg.n_range, cfg.n_chirps, cfg.n_rx, cfg.n_tx = N_RANGE, N_CHIRPS, N_RX, N_TX
        cfg.align = _ALIGN[align] if isinstance(align, str) else align
        cfg.device_id = device
        self._create(cfg)

    @property
    def n_virtual(self) -> int:
        """Channels of the output: n_tx * n_rx."""
        return self.cfg.n_tx * self.cfg.n_rx

    @property
    def n_d(self) -> int:
        """Chirps per channel of the output: n_chirps / n_tx."""
        return self.cfg.n_chirps // self.cfg.n_tx

    def frame_bytes(self) -> int:
        """Of one frame of the input, and of the output."""
        c = self.cfg
        return c.n_rx * c.n_range * c.n_chirps * 8

    def enqueue(self, spec, n_frames: int, out, stream: int = 0):
        """Asynchronous, device pointers only (DeviceBuffer / torch CUDA tensors / ints).  spec: n_frames
        frames of range_ct output; out: as many bytes, 16-byte aligned, not overlapping spec."""
        L.check(self._lib.fmcw_mimo_enqueue(self._h, ptr(spec), n_frames, ptr(out), stream or None))

    def form(self, spec) -> np.ndarray:
        """Synchronous.  spec: range_ct output as a DeviceBuffer / CUDA tensor, or a host complex64 array
        [frame][rx][range][chirp].  Returns complex64 [frame][n_tx * n_rx][range][n_d]."""
        c = self.cfg
        own = []
        try:
            spec, nbytes = stage(spec, np.complex64, 16, self.device, own)
            nf, rem = divmod(nbytes, self.frame_bytes())
            if rem:
                raise ValueError(f"spectrum of {nbytes} B is not a whole number of frames ({self.frame_bytes()} B each)")
            do = DeviceBuffer(max(nf * self.frame_bytes(), 16), self.device)
            own.append(do)
            self.enqueue(spec, nf, do)
            # fmcw_memcpy is synchronous on the default stream the call ran on
            return do.download(np.complex64, (nf, self.n_virtual, c.n_range, self.n_d))
        finally:
            for b in own:
                b.free()

    def set_grid_for_test(self, grid: int) -> None:
        """fmcw_mimo_set_grid_for_test: at most `grid` workgroups (0: the built-in bound), so that a small
        call drives a workgroup through several tiles, channels and frames."""
        super().set_grid_for_test(grid)
