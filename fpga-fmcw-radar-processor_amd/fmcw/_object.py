"""What the wrappers of the objects beside RadarCore share (private): the handle's life cycle, the pointer
argument of their enqueue calls, the staging of a host array and the run-twice loops of the detectors
and of the list-in / list-out objects."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from .radar_core import DET_DTYPE, DeviceBuffer, _ptr


def ptr(x):
    """The pointer argument of an enqueue call: an int or None as it is, else the address of a
    DeviceBuffer / torch CUDA tensor."""
    return x if isinstance(x, int) or x is None else _ptr(x)[0]


class DeviceObject:
    """A handle made by <_SYM>_create and released by <_SYM>_destroy, with <_SYM>_set_grid_for_test."""
    _SYM = ""   # "fmcw_cacfar", ...

    def _default_config(self, cfg_type):
        """Loads the library; returns a cfg_type filled by <_SYM>_config_default."""
        self._lib = L.load()
        cfg = cfg_type()
        getattr(self._lib, self._SYM + "_config_default")(C.byref(cfg))
        return cfg

    def _create(self, cfg, *args) -> None:
        """self.cfg, self.device, and self._h from <_SYM>_create(&cfg, *args, &handle)."""
        self.cfg = cfg
        self.device = cfg.device_id
        h = C.c_void_p()
        L.check(getattr(self._lib, self._SYM + "_create")(C.byref(cfg), *args, C.byref(h)))
        self._h = h

    def set_grid_for_test(self, grid: int) -> None:
        """At most `grid` workgroups for the object's tile kernels (0: the built-in bound)."""
        L.check(getattr(self._lib, self._SYM + "_set_grid_for_test")(self._h, int(grid)))

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            getattr(self._lib, self._SYM + "_destroy")(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def stage(x, dtype, min_bytes: int, device: int, own: list):
    """(device buffer, bytes) of x: a host array is uploaded as `dtype` into a DeviceBuffer of at least
    min_bytes that is appended to `own` (the caller frees it); a DeviceBuffer / CUDA tensor passes."""
    if isinstance(x, np.ndarray):
        host = np.ascontiguousarray(x, dtype=dtype)
        dev = DeviceBuffer(max(host.nbytes, min_bytes), device)
        own.append(dev)
        if host.nbytes:
            dev.upload(host)
        return dev, host.nbytes
    return x, x.nbytes if isinstance(x, DeviceBuffer) else x.numel() * x.element_size()


def detect_maps(det, maps, det_cap, changed: str, before_rerun=None) -> np.ndarray:
    """The synchronous detect() of a map detector `det` (map_frame_bytes, enqueue, device): stages the
    maps, counts whole frames and runs, once more with the reported count when the first capacity was
    short -- after before_rerun(), if given.  `changed`: the RuntimeError text should the count differ
    between the two runs."""
    own = []
    try:
        maps, nbytes = stage(maps, np.float32, 16, det.device, own)
        nf, rem = divmod(nbytes, det.map_frame_bytes())
        if rem:
            raise ValueError(f"maps of {nbytes} B are not a whole number of frames ({det.map_frame_bytes()} B each)")
        cap = max(nf * 4096, 64) if det_cap is None else det_cap
        dn = DeviceBuffer(4 * L.STATUS_WORDS, det.device)
        own.append(dn)
        for attempt in range(2):
            dd = DeviceBuffer(max(cap, 1) * DET_DTYPE.itemsize, det.device)
            try:
                det.enqueue(maps, nf, dd, cap, dn)
                # fmcw_memcpy is synchronous on the default stream the call ran on
                found = int(dn.download(np.uint32, (L.STATUS_WORDS,))[0])
                if found <= cap:
                    return dd.download(DET_DTYPE, (found,))
            finally:
                dd.free()
            if attempt == 0 and before_rerun:
                before_rerun()
            cap = found
        raise RuntimeError(changed)
    finally:
        for b in own:
            b.free()


def run_list(obj, recs: np.ndarray, count_words: int, status_words: int, out_dtype, cap: int, enqueue, changed: str):
    """The synchronous call of a list-in / list-out object `obj` (device): uploads the contiguous host
    records and their count word (the first of count_words uint32) and runs enqueue(recs_dev, n,
    count_dev, out_dev, cap, status_dev), once more with the reported count when cap was short.  Returns
    (host out_dtype records, the status_words status words).  `changed`: the RuntimeError text should
    the count differ between the two runs."""
    n = len(recs)
    dr = DeviceBuffer(max(n, 1) * recs.dtype.itemsize, obj.device)
    dn = DeviceBuffer(4 * count_words, obj.device)
    ds = DeviceBuffer(4 * status_words, obj.device)
    try:
        if n:
            dr.upload(recs)
        count = np.zeros(count_words, np.uint32)
        count[0] = n
        dn.upload(count)
        for _ in range(2):
            do = DeviceBuffer(max(cap, 1) * out_dtype.itemsize, obj.device)
            try:
                enqueue(dr, n, dn, do, cap, ds)
                # fmcw_memcpy is synchronous on the default stream the call ran on
                status = ds.download(np.uint32, (status_words,))
                found = int(status[0])
                if found <= cap:
                    return do.download(out_dtype, (found,)), status
            finally:
                do.free()
            cap = found
        raise RuntimeError(changed)
    finally:
        dr.free()
        dn.free()
        ds.free()
