#!/usr/bin/env python3
"""Time the plot extractor (fmcw_plots_enqueue) on the bench's detection lists.

Builds each workload's detection list once through the whole path (bench.py's synthetic frames,
fmcw_enqueue with per-kernel profiling on), then times fmcw_plots_enqueue on that list with stream
events and prints one JSON line per (workload, scale override, window): the mean time per call, the
records and plots, and -- as the yardstick -- the FMCW_K_COMPACT time of the call that produced the
list (the detection-ordering pass: existing code that makes one pass over the same records).
usage: python tools/plots_bench.py [--cases c3:0,c5:0,c5:1] [--windows 1x1,4x4] [--frames 4] [--iters 20]
(a case is workload:cfar_scale_ovr; ovr 1 is the reference's dense list, ~27 % of all cells)"""
import argparse
import json
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "fpga-fmcw-radar-processor_amd"))

GEOM = {"c3": dict(ns=4096, nc=512, nrx=4, dtype="f32"), "c5": dict(ns=8192, nc=1024, nrx=1, dtype="f16")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="c3:0,c5:0,c5:1")
    ap.add_argument("--windows", default="1x1,4x4")
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    import numpy as np
    import torch
    from fmcw import RadarCore, PlotExtractor, synth

    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    for case in a.cases.split(","):
        w, ovr = case.split(":")
        g, ovr, F = GEOM[w], int(ovr), a.frames
        ns, nc, nrx = g["ns"], g["nc"], g["nrx"]
        u = synth.frames(F, ns, nc, nrx, "two_targets", seed=1234, dtype=g["dtype"])
        if g["dtype"] == "f32":
            u = u.view(np.float32)
        cube = torch.from_numpy(np.ascontiguousarray(u)).to(dev)
        cap = F * ns * nc if ovr else F * 65536
        dets = torch.empty((cap, 4), dtype=torch.int32, device=dev)
        nd = torch.zeros(4, dtype=torch.int32, device=dev)
        with RadarCore(N_RANGE=ns, N_DOPPLER=nc, N_RX=nrx, in_dtype=g["dtype"], cfar="os2d", max_frames=F,
                       cfar_scale_ovr=ovr) as core:
            core.enqueue(cube, F, None, dets, cap, nd, stream=stream)   # warm-up
            torch.cuda.synchronize()
            core.set_profiling(True)
            core.reset_kernel_times()
            for _ in range(3):
                core.enqueue(cube, F, None, dets, cap, nd, stream=stream)
            torch.cuda.synchronize()
            kt = core.kernel_times()
        del cube
        compact_us = 1e3 * kt["k_compact"][0] / 3
        n = int(nd[0].item())
        assert n <= cap and int(nd[1].item()) == 0, nd
        for win in a.windows.split(","):
            wr, wd = (int(x) for x in win.split("x"))
            pcap = max(n, 1)
            plots = torch.empty((pcap, 8), dtype=torch.int32, device=dev)
            st = torch.zeros(2, dtype=torch.int32, device=dev)
            with PlotExtractor(ns, nc, win=(wr, wd), max_dets=max(n, 1)) as px:
                for _ in range(3):
                    px.enqueue(dets, cap, nd, plots, pcap, st, stream=stream)
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.iters):
                    px.enqueue(dets, cap, nd, plots, pcap, st, stream=stream)
                e1.record()
                torch.cuda.synchronize()
                us = 1e3 * e0.elapsed_time(e1) / a.iters
            print(json.dumps({"workload": w, "ovr": ovr, "frames": F, "window": [wr, wd], "n_dets": n,
                              "n_plots": int(st[0].item()), "not_examined": int(st[1].item()),
                              "plots_us_per_call": round(us, 1), "k_compact_us_per_call": round(compact_us, 1),
                              "ratio": round(us / max(compact_us, 1e-9), 2),
                              "ns_per_det": round(1e3 * us / max(n, 1), 3)}), flush=True)
            del plots
        del dets


if __name__ == "__main__":
    main()
