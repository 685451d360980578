#!/usr/bin/env python3
"""Time the clutter map (fmcw_cmap_enqueue) beside the cell-averaging detector (fmcw_cacfar_enqueue) on
the same maps in one process: the config-3 (4096 x 512) and config-5 (8192 x 1024) map shapes, 16 frames
per launch, one stream, the default spread 1/1, on the bench's own map and the clutter maps of
tools/cfar2d_bench.py --maps.

Per (workload, map, detector): 3 warm-up launches, then `--iters` launches between two stream events.  The
clutter map's state advances with every launch, so every timed launch runs with all ages past the warm-up:
each scan tests every cell.  One JSON line each: us per launch, detections of the last launch, and for the
clutter map the fraction of 8 TB/s that its model bytes would need in that time: 8 B per cell per frame
(the two reads of the maps) plus 8 B per cell per call (one read and one write of the state).
usage: python tools/cmap_bench.py [--workloads c3,c5] [--iters 20] [--maps bench,exponential,lognormal,sparse]"""
import argparse
import json
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "fpga-fmcw-radar-processor_amd"))
sys.path.insert(0, str(REPO / "tools"))

from cacfar_bench import timed  # noqa: E402
from cfar2d_bench import GEOM, clutter  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="c3,c5")
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--maps", default="bench,exponential,lognormal,sparse")
    a = ap.parse_args()
    import numpy as np
    import torch
    from fmcw import CaCfar, ClutterMap, RadarCore, synth

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
            with ClutterMap(ns, nc, max_frames=F) as cm:
                us = timed(lambda: cm.enqueue(m, F, dets, cap, nd, stream=stream), a.iters)
                n = int(nd[0].item())
            need = 8 * cells + 8 * ns * nc
            print(json.dumps({**tag, "detector": "cmap", "us_per_launch": round(us, 1), "n_dets": n, "det_cap": cap,
                              "model_bytes": need, "fraction_of_8TBps": round(need / (us * 1e-6) / 8e12, 4)}), flush=True)
            with CaCfar(ns, nc, mode="ca", max_frames=F) as det:
                us = timed(lambda: det.enqueue(m, F, dets, cap, nd, stream=stream), a.iters)
                n = int(nd[0].item())
            need = 4 * cells + 16 * min(n, cap)
            print(json.dumps({**tag, "detector": "ca", "us_per_launch": round(us, 1), "n_dets": n, "det_cap": cap,
                              "compulsory_bytes": need, "fraction_of_8TBps": round(need / (us * 1e-6) / 8e12, 4)}),
                  flush=True)
            m = None
        del bench_map, dets


if __name__ == "__main__":
    main()
