#!/usr/bin/env python3
"""Time the cell-averaging detector (fmcw_cacfar_enqueue) beside the 2-D OS-CFAR (fmcw_cfar) on the
same maps in one process: the config-3 (4096 x 512) and config-5 (8192 x 1024) map shapes, 16 frames
per launch, the bench's own map and the clutter maps of tools/cfar2d_bench.py --maps.

Per (workload, map, detector): 3 warm-up launches, then `--iters` launches between two stream events.
One JSON line each: us per launch, detections, and for the cell-averaging detector the fraction of
8 TB/s that its compulsory bytes (4 B per cell + 16 B per record) would need in that time.
usage: python tools/cacfar_bench.py [--workloads c3,c5] [--iters 20] [--modes ca,go,so]
                                   [--maps bench,exponential,lognormal,sparse]"""
import argparse
import json
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "fpga-fmcw-radar-processor_amd"))
sys.path.insert(0, str(REPO / "tools"))

from cfar2d_bench import GEOM, clutter  # noqa: E402


def timed(fn, iters):
    import torch
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="c3,c5")
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--modes", default="ca,go,so")
    ap.add_argument("--maps", default="bench,exponential,lognormal,sparse")
    a = ap.parse_args()
    import numpy as np
    import torch
    from fmcw import CaCfar, RadarCore, synth

    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    for w in a.workloads.split(","):
        g = GEOM[w]
        F, ns, nc, nrx = a.frames, g["ns"], g["nc"], g["nrx"]
        cells = F * ns * nc
        cap = cells // 4
        dets = torch.empty((cap, 4), dtype=torch.int32, device=dev)
        nd = torch.zeros(4, dtype=torch.int32, device=dev)
        u = synth.frames(min(16, F), ns, nc, nrx, "two_targets", seed=1234, dtype=g["dtype"])
        if g["dtype"] == "f32":
            u = u.view(np.float32)
        ut = torch.from_numpy(np.ascontiguousarray(u)).to(dev)
        cube = ut.repeat((F // ut.shape[0],) + (1,) * (ut.dim() - 1)).contiguous()
        del ut
        bench_map = torch.empty((F, ns, nc), dtype=torch.float32, device=dev)
        with RadarCore(N_RANGE=ns, N_DOPPLER=nc, N_RX=nrx, in_dtype=g["dtype"], cfar="none", max_frames=F) as core:
            core.enqueue(cube, F, bench_map, stream=stream)
            torch.cuda.synchronize()
        del cube
        for mp in a.maps.split(","):
            m = bench_map if mp == "bench" else clutter(mp, F, ns, nc, dev)
            tag = {"workload": w, "map": mp, "frames": F, "n_range": ns, "n_doppler": nc}
            for mode in a.modes.split(","):
                with CaCfar(ns, nc, mode=mode, max_frames=F) as det:
                    us = timed(lambda: det.enqueue(m, F, dets, cap, nd, stream=stream), a.iters)
                    n = int(nd[0].item())
                need = 4 * cells + 16 * min(n, cap)
                print(json.dumps({**tag, "detector": mode, "us_per_launch": round(us, 1), "n_dets": n,
                                  "det_cap": cap, "compulsory_bytes": need,
                                  "fraction_of_8TBps": round(need / (us * 1e-6) / 8e12, 4)}), flush=True)
            with RadarCore(N_RANGE=ns, N_DOPPLER=nc, N_RX=1, cfar="os2d", max_frames=F) as core:
                us = timed(lambda: core.cfar(m, F, dets, cap, nd, stream=stream), a.iters)
                print(json.dumps({**tag, "detector": "os2d (K3)", "us_per_launch": round(us, 1),
                                  "n_dets": int(nd[0].item()), "lost": int(nd[1].item())}), flush=True)
            m = None
        del bench_map, dets


if __name__ == "__main__":
    main()
