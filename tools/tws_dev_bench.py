#!/usr/bin/env python3
"""Time fmcw_tws_dev_enqueue alone on a resident list against the host path on the same list.

    python tools/tws_dev_bench.py [--repeats 30] [--warmup 5] [--rtl] [--gate R D]

Three cases: 1024 scans x 1 stream at about 8 detections per scan, the same at 64 per scan, and
16 scans x 64 streams at about 8.  Per case, one JSON line with
  gpu_us        fmcw_tws_dev_enqueue (both kernels), device events around one call, the track files
                reset before every call outside the timed window: median, min, max over the repeats.
                The first event is recorded before the Python call, so this includes the host's two
                launches through ctypes, during which the device is idle
  gpu_b2b_us    per call, ten calls enqueued back to back between the two events (the launches of
                the later calls overlap the kernels of the earlier ones; the track files run on
                from call to call): median, min, max
  host_us       what a caller did before: the device-to-host copy of the list, then one fmcw_tws_scan
                per (scan, stream) through ctypes on slices of the downloaded buffer (no per-detection
                Python work): host clock, median, min, max
  host_class_us the same loop through TwsTracker.scan as shipped (it fills a ctypes struct per
                detection): one timed pass after a warm-up pass
The results of the two paths are compared before anything is timed.  Needs an MI355X.
"""
import argparse
import ctypes as C
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "fpga-fmcw-radar-processor_amd"))

from fmcw import DET_DTYPE, TRACK_DTYPE, DeviceBuffer, DeviceTwsTracker, TwsTracker  # noqa: E402
from fmcw import _lib as L  # noqa: E402


def make_list(n_scans, n_streams, per_scan, seed):
    """Six drifting targets per stream seen with probability 0.85 plus clutter up to about per_scan
    detections per (scan, stream); frame = scan * n_streams + stream."""
    rng = np.random.default_rng(seed)
    rows = []
    tgt = rng.integers([20, 5], [1000, 120], (n_streams, 6, 2)).astype(np.int64)
    vel = rng.integers([-3, -1], [4, 2], (n_streams, 6, 2))
    for k in range(n_scans):
        tgt = np.clip(tgt + vel + rng.integers(-1, 2, tgt.shape), 0, [1023, 127])
        for s in range(n_streams):
            seen = tgt[s][rng.random(6) < 0.85]
            n_clutter = per_scan - len(seen) if per_scan >= 64 else int(rng.integers(0, max(1, 2 * (per_scan - 5) + 1)))
            clutter = np.stack([rng.integers(0, 1024, n_clutter), rng.integers(0, 128, n_clutter)], 1)
            d = np.concatenate([seen, clutter])
            rng.shuffle(d)
            rows += [(k * n_streams + s, int(r), int(c), float(rng.integers(100, 200000))) for r, c in d]
    a = np.zeros(len(rows), DET_DTYPE)
    f, r, d, m = zip(*rows)
    a["frame"], a["range"], a["doppler"], a["mag"] = f, r, d, m
    return a


class Events:
    def __init__(self):
        self.hip = C.CDLL("libamdhip64.so")
        self.hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
        self.hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
        self.hip.hipEventSynchronize.argtypes = [C.c_void_p]
        self.a, self.b = C.c_void_p(), C.c_void_p()
        for e in (self.a, self.b):
            assert self.hip.hipEventCreate(C.byref(e)) == 0

    def time_us(self, fn):
        assert self.hip.hipEventRecord(self.a, None) == 0
        fn()
        assert self.hip.hipEventRecord(self.b, None) == 0
        assert self.hip.hipEventSynchronize(self.b) == 0
        ms = C.c_float()
        assert self.hip.hipEventElapsedTime(C.byref(ms), self.a, self.b) == 0
        return ms.value * 1e3


def host_loop(lib, handles, buf, bounds, n_streams, out):
    """One fmcw_tws_scan per (scan, stream) on slices of the downloaded list."""
    n_out, n_act = C.c_size_t(0), C.c_uint32(0)
    base, res = buf.ctypes.data, []
    for m in range(len(bounds) - 1):
        b, e = bounds[m], bounds[m + 1]
        lib.fmcw_tws_scan(handles[m % n_streams], C.c_void_p(base + 16 * b), e - b, out, len(out), C.byref(n_out),
                          C.byref(n_act))
        res.append((n_out.value, n_act.value))
    return res


def stats(x):
    return dict(median=round(statistics.median(x), 1), min=round(min(x), 1), max=round(max(x), 1), n=len(x))


def bench_case(name, n_scans, n_streams, per_scan, a, ev):
    lib = L.load()
    recs = make_list(n_scans, n_streams, per_scan, seed=n_streams + per_scan)
    n, groups, cap = len(recs), n_scans * n_streams, 32
    bounds = np.searchsorted(recs["frame"], np.arange(groups + 1)).tolist()
    dr, dn = DeviceBuffer(recs.nbytes), DeviceBuffer(16)
    dt, dc, ds = DeviceBuffer(groups * cap * 28), DeviceBuffer(groups * 8), DeviceBuffer(8)
    dr.upload(recs)
    dn.upload(np.array([n, 0, 0, 0], np.uint32))

    def new_host():
        hs = []
        cfg = L.FmcwTwsConfig()
        lib.fmcw_tws_config_default(C.byref(cfg))
        cfg.rtl_compat = int(a.rtl)
        cfg.gate_r, cfg.gate_d = a.gate
        for _ in range(n_streams):
            h = C.c_void_p()
            L.check(lib.fmcw_tws_create(C.byref(cfg), C.byref(h)))
            hs.append(h)
        return hs

    def free_host(hs):
        for h in hs:
            lib.fmcw_tws_destroy(h)

    out = (L.FmcwTrack * cap)()
    with DeviceTwsTracker(n_streams=n_streams, max_scans=n_scans, rtl_compat=a.rtl, ASSOC_GATE_R=a.gate[0],
                          ASSOC_GATE_D=a.gate[1]) as trk:
        def call():
            trk.enqueue(dr, 16, n, dn, n_scans, dt, cap, dc, ds)
        # the two paths agree on every count before anything is timed
        call()
        counts = dc.download(np.uint32, (groups, 2))
        hs = new_host()
        want = host_loop(lib, hs, dr.download(DET_DTYPE, (n,)), bounds, n_streams, out)
        free_host(hs)
        assert [tuple(c) for c in counts.tolist()] == want, name
        gpu = []
        for k in range(a.warmup + a.repeats):
            trk.reset()
            t = ev.time_us(call)
            if k >= a.warmup:
                gpu.append(t)

        def ten():
            for _ in range(10):
                call()
        b2b = []
        for k in range(2 + max(3, a.repeats // 3)):
            trk.reset()
            t = ev.time_us(ten) / 10
            if k >= 2:
                b2b.append(t)
    host = []
    for k in range(2 + max(3, a.repeats // 3)):
        hs = new_host()
        t0 = time.perf_counter()
        buf = dr.download(DET_DTYPE, (n,))
        host_loop(lib, hs, buf, bounds, n_streams, out)
        t1 = time.perf_counter()
        free_host(hs)
        if k >= 2:
            host.append((t1 - t0) * 1e6)
    cls = None
    for k in range(2):
        trks = [TwsTracker(rtl_compat=a.rtl, ASSOC_GATE_R=a.gate[0], ASSOC_GATE_D=a.gate[1]) for _ in range(n_streams)]
        t0 = time.perf_counter()
        buf = dr.download(DET_DTYPE, (n,))
        for m in range(groups):
            trks[m % n_streams].scan(buf[bounds[m]:bounds[m + 1]])
        cls = (time.perf_counter() - t0) * 1e6
        for t in trks:
            t.close()
    for b in (dr, dn, dt, dc, ds):
        b.free()
    g, h = stats(gpu), stats(host)
    lib_name = Path(str(L.LIB_PATH)).name
    print(json.dumps(dict(case=name, scans=n_scans, streams=n_streams, records=n, rtl=bool(a.rtl), gate=list(a.gate), lib=lib_name, gpu_us=g,
                          gpu_b2b_us=stats(b2b), host_us=h,
                          host_class_us=round(cls, 1), gpu_us_per_scan=round(g["median"] / groups, 3),
                          host_us_per_scan=round(h["median"] / groups, 3))), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--gate", type=int, nargs=2, default=[10, 5], metavar=("R", "D"),
                    help="association gate in range and Doppler bins (4096 4096: every detection is a candidate)")
    ap.add_argument("--rtl", action="store_true", help="both trackers in RTL-compat mode")
    a = ap.parse_args()
    if L.device_count() < 1:
        raise SystemExit("tws_dev_bench needs an MI355X: no HIP device is visible")
    ev = Events()
    bench_case("1024x1 ~8", 1024, 1, 8, a, ev)
    bench_case("1024x1 64", 1024, 1, 64, a, ev)
    bench_case("16x64 ~8", 16, 64, 8, a, ev)


if __name__ == "__main__":
    main()
