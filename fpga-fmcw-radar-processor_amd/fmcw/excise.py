"""Interference excision on the ADC cube (ctypes over fmcw_excise_*, include/fmcw.h).

Another FMCW radar's chirp crossing ours leaves a short burst in some chirps, far above the noise; it is
white in range, so it raises the whole range-Doppler map and every CFAR adapts to it.
``InterferenceExciser`` finds the burst per chirp against an exact order statistic of the chirp's own
power (the median by default), widens the flags by a guard and zeroes or linearly interpolates every run,
before the window and the range FFT.  The repaired cube has the layout and dtype of the input, so
``RadarCore.enqueue`` / ``range_ct`` take it as it is.  The rule is specified exactly in include/fmcw.h.
"""
from __future__ import annotations

import numpy as np

from . import _lib as L
from ._object import DeviceObject, ptr, stage
from .radar_core import _IN_DTYPES, DeviceBuffer

_MODES = {"zero": L.EXCISE_ZERO, "interp": L.EXCISE_INTERP}


class InterferenceExciser(DeviceObject):
    _SYM = "fmcw_excise"

    def __init__(self, N_RANGE: int = 1024, N_DOPPLER: int = 128, n_rx: int = 1, in_dtype: str = "f32",
                 mode: str = "zero", guard: int = 4, rank_pct: int = 50, alpha: float = 16.0, max_frames: int = 1,
                 device: int = 0):
        """mode: "zero" blanks every run, "interp" interpolates linearly between the run's neighbours.
        guard: samples added on each side of a flagged sample (0..32).  rank_pct: the rank of the level
        among the chirp's powers (1..99, 50 = the median).  alpha: power ratio over the level above
        which a sample is flagged (finite, >= 1).  in_dtype: "f32", "f16" or "i16", as RadarCore's."""
        cfg = self._default_config(L.FmcwExciseConfig)
        cfg.n_range, cfg.n_doppler, cfg.n_rx = N_RANGE, N_DOPPLER, n_rx
        cfg.in_dtype = _IN_DTYPES[in_dtype][0] if isinstance(in_dtype, str) else in_dtype
        cfg.mode = _MODES[mode] if isinstance(mode, str) else mode
        cfg.guard, cfg.rank_pct, cfg.alpha = guard, rank_pct, alpha
        cfg.max_frames, cfg.device_id = max_frames, device
        self.in_dtype = {v[0]: k for k, v in _IN_DTYPES.items()}.get(cfg.in_dtype, "f32")
        self._create(cfg)

    def lines_per_frame(self) -> int:
        return self.cfg.n_rx * self.cfg.n_doppler

    def frame_bytes(self) -> int:
        return self.lines_per_frame() * self.cfg.n_range * (8 if self.in_dtype == "f32" else 4)

    def enqueue(self, cube, n_frames: int, out, mask, counts, status, stream: int = 0):
        """Asynchronous, device pointers only (DeviceBuffer / torch CUDA tensors / ints).  cube: n_frames
        frames [rx][chirp][sample]; out: the repaired cube, `cube` itself (in place) or disjoint from
        it; mask: n_range / 32 uint32 words per chirp, or None; counts: one uint32 per chirp, or None;
        status: FMCW_EXCISE_STATUS_WORDS (4) uint32 words: samples repaired, chirps repaired, samples
        flagged before the guard, chirps with more than half their samples repaired."""
        L.check(self._lib.fmcw_excise_enqueue(self._h, ptr(cube), n_frames, ptr(out), ptr(mask), ptr(counts),
                                              ptr(status), stream or None))

    def repair(self, cube):
        """Synchronous.  cube: a host array in RadarCore's conventions (complex64 [frame][rx][chirp]
        [sample], or float16 / int16 with a last axis of 2), or a DeviceBuffer / CUDA tensor holding
        whole frames.  Returns (the repaired cube, shaped as a host input was; the mask as bool
        [frame][rx][chirp][sample]; the counts [frame][rx][chirp]; the four status words)."""
        c = self.cfg
        np_dtype = _IN_DTYPES[self.in_dtype][1]
        own = []
        try:
            dev, nbytes = stage(cube, np_dtype, 16, self.device, own)
            nf, rem = divmod(nbytes, self.frame_bytes())
            if rem or nf < 1:
                raise ValueError(f"cube of {nbytes} B is not a whole number of frames ({self.frame_bytes()} B each)")
            lines = nf * self.lines_per_frame()
            do = DeviceBuffer(nbytes, self.device)
            dm = DeviceBuffer(lines * c.n_range // 8, self.device)
            dc = DeviceBuffer(lines * 4, self.device)
            ds = DeviceBuffer(4 * L.EXCISE_STATUS_WORDS, self.device)
            own += [do, dm, dc, ds]
            self.enqueue(dev, nf, do, dm, dc, ds)
            # fmcw_memcpy is synchronous on the default stream the call ran on
            status = ds.download(np.uint32, (L.EXCISE_STATUS_WORDS,))
            counts = dc.download(np.uint32, (nf, c.n_rx, c.n_doppler))
            words = dm.download(np.uint8, (nf, c.n_rx, c.n_doppler, c.n_range // 8))
            mask = np.unpackbits(words, axis=-1, bitorder="little").astype(bool)
            shape = cube.shape if isinstance(cube, np.ndarray) else \
                (nf, c.n_rx, c.n_doppler, c.n_range) + (() if self.in_dtype == "f32" else (2,))
            return do.download(np_dtype, shape), mask, counts, status
        finally:
            for b in own:
                b.free()

    def set_grid_for_test(self, grid: int) -> None:
        """fmcw_excise_set_grid_for_test: at most `grid` workgroups (0: the built-in bound), so that a
        small call drives a workgroup through several chirps."""
        super().set_grid_for_test(grid)
