"""What the GPU tests share: the HIP graph binding, the path helpers, the sentinel vocabulary, the run helpers
of the list objects and the tracker-chain fixtures.  A helper, not a test module: it imports on a machine
without a GPU and loads neither libamdhip64.so nor libfmcw.so until a helper is called.

pytest does not rewrite the asserts of a helper module, so every assert here carries its own message
with the compared values.
"""
import contextlib
import ctypes as C
import functools
import subprocess
import sys

import numpy as np
import pytest

import fmcw_oracle as O
import scenario_ref as S
import tws_dev_ref as TR
from conftest import PKG, rel_err
from fmcw import (DET_DTYPE, PLOT_DTYPE, TRACK_DTYPE, DeviceBuffer, DeviceTwsTracker, PlotExtractor, RadarCore)

# ---- the sentinel vocabulary -------------------------------------------------------------------
SENTINEL = 0xA5               # the byte every output buffer is filled with before a run
GUARD = 0xA5A5A5A5            # a word of it, around status words
SENTINEL_WORD = GUARD         # as a float32 -2.9e-16: finite, and a zero for any tolerance


def sentinel_buffer(nbytes, device=0):
    """A device buffer of nbytes (at least 8) sentinel bytes."""
    nbytes = max(int(nbytes), 8)
    d = DeviceBuffer(nbytes, device)
    d.upload(np.full(nbytes, SENTINEL, np.uint8))
    return d


def assert_sentinel_after(raw, n=0, rec_bytes=1, what="the output"):
    """Every byte of `raw` (any dtype, read as bytes) after its first n records of rec_bytes still holds the
    sentinel.  With n = 0 it is the check of guard words and of a buffer that must stay untouched."""
    rest = np.ascontiguousarray(raw).reshape(-1).view(np.uint8)[n * rec_bytes:]
    bad = np.flatnonzero(rest != SENTINEL)
    assert bad.size == 0, (f"{what}: {bad.size} of the {rest.size} bytes after the first {n} records of {rec_bytes} bytes "
                           f"were written, the first at byte {n * rec_bytes + int(bad[0])} = {int(rest[bad[0]]):#04x}")


def assert_all_written(raw, what):
    """No 32-bit word of a float output (its bytes, a multiple of 4) still holds the sentinel the buffer
    was filled with.  A genuine value with that bit pattern is -2.9e-16, which no scene here produces."""
    left = np.flatnonzero(np.ascontiguousarray(raw).view(np.uint32) == SENTINEL_WORD)
    assert left.size == 0, f"{what}: {left.size} words were never written, the first at word {left[0]}"


# ---- hipGraph capture -------------------------------------------------------------------------
class Hip:
    """The few HIP runtime calls a graph capture needs, bound with ctypes (no torch)."""
    CAPTURE_RELAXED = 2   # hipStreamCaptureModeRelaxed

    def __init__(self):
        self.lib = C.CDLL("libamdhip64.so")
        for name in ("hipStreamCreate", "hipStreamDestroy", "hipStreamBeginCapture", "hipStreamEndCapture",
                     "hipGraphInstantiate", "hipGraphLaunch", "hipGraphExecDestroy", "hipGraphDestroy",
                     "hipStreamSynchronize"):
            getattr(self.lib, name).restype = C.c_int
        self.lib.hipStreamBeginCapture.argtypes = [C.c_void_p, C.c_int]
        self.lib.hipStreamEndCapture.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
        self.lib.hipGraphInstantiate.argtypes = [C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p, C.c_void_p,
                                                 C.c_size_t]
        self.lib.hipGraphLaunch.argtypes = [C.c_void_p, C.c_void_p]
        self.lib.hipStreamSynchronize.argtypes = [C.c_void_p]
        self.lib.hipStreamDestroy.argtypes = [C.c_void_p]
        self.lib.hipGraphExecDestroy.argtypes = [C.c_void_p]
        self.lib.hipGraphDestroy.argtypes = [C.c_void_p]

    def ok(self, rc):
        assert rc == 0, f"HIP error {rc}"

    def stream(self):
        s = C.c_void_p()
        self.ok(self.lib.hipStreamCreate(C.byref(s)))
        return s

    def capture(self, s, fn):
        self.ok(self.lib.hipStreamBeginCapture(s, self.CAPTURE_RELAXED))
        try:
            fn()
        finally:
            g = C.c_void_p()
            rc = self.lib.hipStreamEndCapture(s, C.byref(g))
        self.ok(rc)
        exe = C.c_void_p()
        self.ok(self.lib.hipGraphInstantiate(C.byref(exe), g, None, None, 0))
        return g, exe

    def replay(self, exe, s):
        self.ok(self.lib.hipGraphLaunch(exe, s))
        self.ok(self.lib.hipStreamSynchronize(s))

    @contextlib.contextmanager
    def graph(self, calls, stream=None):
        """calls(s) captured on stream s (a new one unless `stream` is given) and instantiated: yields
        (exe, s) for replay(exe, s).  On exit, by a failed assertion too, the exec and the graph are
        destroyed, and the stream if it was made here."""
        s = self.stream() if stream is None else stream
        g = exe = None
        try:
            g, exe = self.capture(s, lambda: calls(s))
            yield exe, s
        finally:
            if exe:
                self.lib.hipGraphExecDestroy(exe)
            if g:
                self.lib.hipGraphDestroy(g)
            if stream is None:
                self.lib.hipStreamDestroy(s)


# ---- the path: maps, spectra, detection lists ---------------------------------------------------
MAP_TOL = 1e-4


def check_map(gpu, ref, tol=MAP_TOL):
    for f in range(ref.shape[0]):
        e = rel_err(gpu[f], ref[f])
        assert e <= tol, f"frame {f}: max rel err {e:.3g}"
        big = np.abs(ref[f]) >= 1e-3 * np.abs(ref[f]).max()
        pb = np.max(np.abs(gpu[f][big] - ref[f][big]) / np.abs(ref[f][big]))
        assert pb <= tol, f"frame {f}: per-bin rel err {pb:.3g}"


def to_complex(cube, dtype):
    if dtype == "f32":
        return cube.astype(np.complex128)
    x = cube.astype(np.float64)
    return x[..., 0] + 1j * x[..., 1]


def run_range_ct(core, cube, nf):
    c = core.cfg
    din = DeviceBuffer(cube.nbytes)
    din.upload(cube)
    spec = DeviceBuffer(nf * c.n_rx * c.n_range * c.n_doppler * 8)
    core.range_ct(din, spec, nf)
    return spec.download(np.complex64, (nf, c.n_rx, c.n_range, c.n_doppler))


def range_ct_spectrum(cube, nr, nc, nrx, win="hamming"):
    """fmcw_range_ct's spectrum of `cube` on the host (the core is the one the CLI builds)."""
    nf = len(cube)
    with RadarCore(N_RANGE=nr, N_DOPPLER=nc, N_RX=nrx, cfar="os1d", max_frames=nf, window=win) as core:
        dc = DeviceBuffer(cube.nbytes)
        dc.upload(cube)
        ds = DeviceBuffer(nf * nrx * nr * nc * 8)
        core.range_ct(dc, ds, nf)
        spec = ds.download(np.complex64, (nf, nrx, nr, nc))
        dc.free()
        ds.free()
    return spec


def run_cfar_stage(core, mag, cap=1 << 16):
    nf = mag.shape[0]
    dm = DeviceBuffer(mag.nbytes)
    dm.upload(np.ascontiguousarray(mag, np.float32))
    dd = DeviceBuffer(cap * 16)
    dn = DeviceBuffer(16)
    core.cfar(dm, nf, dd, cap, dn)
    n, dropped = (int(x) for x in dn.download(np.uint32, (2,)))
    assert n <= cap and dropped == 0, f"fmcw_cfar: n = {n}, cap = {cap}, dropped = {dropped}"
    return dd.download(DET_DTYPE, (cap,))[:n]


def oracle_dets(mag32, cfar):
    out = []
    for f in range(mag32.shape[0]):
        if isinstance(cfar, O.Cfar1D):
            det, thr = O.cfar_os1d(mag32[f], cfar)
        else:
            det, thr = O.cfar_os2d(mag32[f], cfar)
        out.append(O.detections(det, mag32[f], thr, frame=f))
    return np.concatenate(out) if out else np.empty(0, O.DET_DTYPE)


def rtl_dets(maps, cf):
    out = []
    for f in range(maps.shape[0]):
        if isinstance(cf, O.Cfar1D):
            det, thr = O.cfar_os1d_rtl(maps[f], cf)
        else:
            det, thr = O.cfar_os2d_rtl(maps[f], cf)
        out.append(O.detections_rtl(det, maps[f], thr, frame=f))
    return np.concatenate(out)


@functools.lru_cache(maxsize=None)
def rayleigh(nf, nr, nd, seed):
    m = np.random.default_rng(seed).rayleigh(1.0, (nf, nr, nd)).astype(np.float32)
    m.setflags(write=False)
    return m


def cli(*args):
    return subprocess.run([sys.executable, "-m", "fmcw.cli", *map(str, args)], cwd=str(PKG),
                          capture_output=True, text=True, timeout=300, check=True)


# ---- one enqueue into guarded buffers -----------------------------------------------------------
def run_map_detector(det, maps, det_cap=None, null_dets=False, canary=8):
    """One enqueue of a map detector (fmcw_cacfar_enqueue, fmcw_cmap_enqueue) on host maps: (the records
    written, the four status words), after checking that every record from min(found, det_cap) on, the
    `canary` records behind det_cap included, kept the sentinel."""
    maps = np.ascontiguousarray(maps, np.float32)
    nf = maps.shape[0]
    cap = maps.size if det_cap is None else det_cap
    dm = DeviceBuffer(max(maps.nbytes, 16))
    if maps.nbytes:
        dm.upload(maps)
    dd = sentinel_buffer((cap + canary) * 16)
    dn = sentinel_buffer(16)
    try:
        det.enqueue(dm, nf, None if null_dets else dd, cap, dn)
        st = dn.download(np.uint32, (4,))
        raw = dd.download(np.uint8, ((cap + canary) * 16,))
    finally:
        for b in (dm, dd, dn):
            b.free()
    n = min(int(st[0]), cap)
    assert_sentinel_after(raw, n, 16, f"detection list (status {st.tolist()}, det_cap {cap})")
    return raw[:n * 16].view(DET_DTYPE).copy(), st


def run_rec_list(enqueue, recs, out_dtype, n_status, out_cap, rec_cap=None, n_word=None, guards=(4, 1), slots_after=4):
    """One enqueue of an object that turns a record list into a record list (plots, merge, unfold) on a
    host list.  enqueue(recs_dev, stride, rec_cap, n_recs_dev, out_dev, out_cap, status_ptr) makes the
    call.  The output buffer has slots_after slots beyond out_cap and is filled with the sentinel; the
    n_status status words sit between guards[0] and guards[1] guard words.  Returns (status words, records
    written, the output buffer's bytes after them), after checking that the guard words and those bytes
    kept the sentinel."""
    n, stride, size = len(recs), recs.dtype.itemsize, out_dtype.itemsize
    rec_cap = n if rec_cap is None else rec_cap
    dr = DeviceBuffer(max(n, 1) * stride)
    if n:
        dr.upload(np.ascontiguousarray(recs))
    dn = DeviceBuffer(16)
    dn.upload(np.array([n if n_word is None else n_word, 0, 0, 0], np.uint32))
    slots = out_cap + slots_after
    do = sentinel_buffer(slots * size)
    before, words = guards[0], guards[0] + n_status + guards[1]
    ds = sentinel_buffer(words * 4)
    try:
        enqueue(dr, stride, rec_cap, dn, do, out_cap, ds.ptr + before * 4)
        st = ds.download(np.uint32, (words,))
        raw = do.download(np.uint8, (slots * size,))
    finally:
        for b in (dr, dn, do, ds):
            b.free()
    assert_sentinel_after(st[:before], what="guard words before the status words")
    assert_sentinel_after(st[before + n_status:], what="guard words after the status words")
    st = st[before:before + n_status]
    k = min(int(st[0]), out_cap)
    assert_sentinel_after(raw, k, size, f"output list (status {st.tolist()}, out_cap {out_cap})")
    return st, raw[: k * size].view(out_dtype).copy(), raw[k * size:]


def run_beams(bf, spec, n_frames=None, tail=4096):
    """One fmcw_beams_enqueue on a host spectrum into a sentinel-filled buffer: the maps, after checking
    that the `tail` bytes behind the last map kept the sentinel and that every map cell was written."""
    n_frames = len(spec) if n_frames is None else n_frames
    c = bf.cfg
    nbytes = n_frames * bf.maps_frame_bytes()
    dspec = DeviceBuffer(max(spec.nbytes, 8))
    dspec.upload(spec)
    dm = sentinel_buffer(nbytes + tail)
    bf.enqueue(dspec, n_frames, dm)
    raw = dm.download(np.uint8, (nbytes + tail,))
    dspec.free()
    dm.free()
    assert_sentinel_after(raw, nbytes, 1, "beam maps")
    assert_all_written(raw[:nbytes], "maps")
    return raw[:nbytes].view(np.float32).reshape(n_frames, c.n_beams, c.n_range, c.n_doppler).copy()


# ---- the device tracker and the scenario chain ---------------------------------------------------
GENERICS = dict(max_tracks="MAX_TRACKS", coast_max="COAST_MAX", init_hits="INIT_HITS", gate_r="ASSOC_GATE_R",
                gate_d="ASSOC_GATE_D", alpha_q8="ALPHA_GAIN", beta_q8="BETA_GAIN", max_dets="MAX_DETS")
RTL = pytest.mark.parametrize("rtl", [False, True])


def tracker(n_streams, max_scans, rtl, **params):
    return DeviceTwsTracker(n_streams=n_streams, max_scans=max_scans, rtl_compat=rtl,
                            **{GENERICS[k]: v for k, v in params.items()})


def assert_matches(got, want, want_status, n_streams, track_cap):
    """(status words, counts [groups][2], track bytes [groups][track_cap x 28], the counts' guard words) of
    one fmcw_tws_dev_enqueue against tws_dev_ref's per (scan, stream) output."""
    st, counts, raw, guard = got
    assert list(st) == want_status, f"status words {list(st)}, expected {want_status}"
    assert_sentinel_after(guard, what="guard words after the counts")
    for scan, row in enumerate(want):
        for s, (tracks, active) in enumerate(row):
            m = scan * n_streams + s
            have = (int(counts[m, 0]), int(counts[m, 1]))
            assert have == (len(tracks), active), f"scan {scan} stream {s}: counts {have}, expected {(len(tracks), active)}"
            k = min(len(tracks), track_cap)
            mine = raw[m, :k * 28].view(TRACK_DTYPE)
            assert TR.tracks_equal(mine, tracks[:k]), f"scan {scan} stream {s}: tracks {mine}, expected {tracks[:k]}"
            assert_sentinel_after(raw[m], k, 28, f"scan {scan} stream {s}: track slots")
    if not want:
        assert_sentinel_after(raw, what="track buffer of a call without scans")


def make_core(scene, mti, path, max_frames, **over):
    kw = dict(N_RANGE=scene.ns, N_DOPPLER=scene.nc, in_dtype="i16", cfar="os2d", max_frames=max_frames,
              mti_bypass=(mti == 0), NOTCH_MODE=mti or 2, **scene.generics)
    if path == "int":       # FMCW_COMPAT_MTI needs the canceller on; the Q15 window selects the words anyway
        kw.update(window="q15_rtl", range_shift=S.INT_SHIFT[scene.id, mti],
                  compat_rtl=("cfar", "mti") if mti else ("cfar",))
    kw.update(over)
    return RadarCore(**kw)


class Guarded:
    """A device buffer with TAIL sentinel bytes behind its `nbytes`."""
    TAIL = 64

    def __init__(self, nbytes):
        self.nbytes = nbytes
        self.buf = DeviceBuffer(nbytes + self.TAIL)
        self.fill()

    def fill(self):
        self.buf.upload(np.full(self.nbytes + self.TAIL, SENTINEL, np.uint8))

    @property
    def ptr(self):
        return self.buf.ptr

    def get(self, dtype, shape):
        return self.buf.download(dtype, shape)

    def check(self):
        assert_sentinel_after(self.buf.download(np.uint8, (self.TAIL,), offset=self.nbytes),
                              what=f"the tail of a buffer of {self.nbytes} bytes")

    def free(self):
        self.buf.free()


class Chain:
    """fmcw_enqueue (map and detections), fmcw_plots_enqueue, fmcw_tws_dev_enqueue on one stream, every
    output buffer guarded."""

    def __init__(self, hip, scene, n_frames, n_streams, rtl):
        self.scene, self.nf, self.ns, self.rtl, self.hip = scene, n_frames, n_streams, rtl, hip
        self.max_scans = n_frames // n_streams
        self.cap = 512 * n_frames
        self.frame_bytes = scene.nc * scene.ns * 4
        self.core = make_core(scene, 2, "float", n_frames)
        self.px = PlotExtractor(scene.ns, scene.nc, win=S.PLOT_WIN, max_dets=self.cap)
        self.trk = tracker(n_streams, self.max_scans, rtl, **S.TWS)
        self.cube = DeviceBuffer(n_frames * self.frame_bytes)
        self.map = Guarded(n_frames * scene.ns * scene.nc * 4)
        self.dets, self.n_dets = Guarded(self.cap * 16), Guarded(16)
        self.plots, self.n_plots = Guarded(S.PLOT_CAP * 32), Guarded(8)
        self.tracks = Guarded(n_frames * S.TRACK_CAP * 28)
        self.counts, self.status = Guarded(n_frames * 8), Guarded(8)
        self.stream = hip.stream()

    def outputs(self):
        return (self.map, self.dets, self.n_dets, self.plots, self.n_plots, self.tracks, self.counts, self.status)

    def enqueue(self, first=0, n_frames=None):
        """The three calls on frames first .. first + n_frames of the uploaded cube."""
        nf = self.nf if n_frames is None else n_frames
        s = self.stream.value
        self.core.enqueue(self.cube.ptr + first * self.frame_bytes, nf, self.map.ptr, self.dets.ptr, self.cap,
                          self.n_dets.ptr, stream=s)
        self.px.enqueue(self.dets.ptr, self.cap, self.n_dets.ptr, self.plots.ptr, S.PLOT_CAP, self.n_plots.ptr, stream=s)
        self.trk.enqueue(self.plots.ptr, 32, S.PLOT_CAP, self.n_plots.ptr, nf // self.ns, self.tracks.ptr, S.TRACK_CAP,
                         self.counts.ptr, self.status.ptr, stream=s)

    def clear(self):
        for b in self.outputs():
            b.fill()
        self.hip.ok(self.hip.lib.hipStreamSynchronize(None))

    def sync(self):
        self.hip.ok(self.hip.lib.hipStreamSynchronize(self.stream))

    def result(self, n_frames=None):
        """Everything the three calls wrote, downloaded after the last of them."""
        nf = self.nf if n_frames is None else n_frames
        self.sync()
        for b in self.outputs():
            b.check()
        st = self.n_dets.get(np.uint32, (4,))
        ps = self.n_plots.get(np.uint32, (2,))
        assert st[0] <= self.cap and st[1] == 0 and ps[0] <= S.PLOT_CAP and ps[1] == 0, \
            f"detection status {st.tolist()} (cap {self.cap}), plot status {ps.tolist()} (cap {S.PLOT_CAP})"
        return dict(map=self.map.get(np.float32, (nf, self.scene.ns, self.scene.nc)),
                    dets=self.dets.get(DET_DTYPE, (int(st[0]),)), plots=self.plots.get(PLOT_DTYPE, (int(ps[0]),)),
                    counts=self.counts.get(np.uint32, (nf, 2)), raw=self.tracks.get(np.uint8, (nf, S.TRACK_CAP * 28)),
                    status=self.status.get(np.uint32, (2,)))

    def close(self):
        self.hip.lib.hipStreamDestroy(self.stream)
        for x in (self.core, self.px, self.trk):
            x.close()
        for b in self.outputs() + (self.cube,):
            b.free()
