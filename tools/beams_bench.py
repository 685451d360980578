#!/usr/bin/env python3
"""Time the beamformer (fmcw_beams_enqueue) on the bench's geometries.

Builds each case's corner-turned spectrum once with fmcw_range_ct (bench.py's synthetic frames), then
times fmcw_beams_enqueue with stream events (3 warm-up calls, then --iters calls between two events)
and prints one JSON line per (case, beam count): the mean time per launch, the compulsory bytes of a
launch (8 n_rx + 4 n_beams per range-Doppler cell and frame: every channel read once, every map
written once) over that time, and that rate as a fraction of the 8 TB/s HBM peak -- the figure the
README gives for K2 (0.68-0.70 at config 3).  A second beam count (default 1) shows what a further
beam costs: its map store, its transform and its re-read of the channels from L2.
usage: python tools/beams_bench.py [--cases c3:3,c2x4:48] [--beams 8,1] [--iters 20]
(a case is geometry:frames; c3 = 512 chirps x 4096 samples x 4 rx, c2x4 = config 2's 256 x 1024 with 4 rx)"""
import argparse
import json
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "fpga-fmcw-radar-processor_amd"))

GEOM = {"c3": dict(ns=4096, nc=512, nrx=4), "c2x4": dict(ns=1024, nc=256, nrx=4)}
HBM_PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="c3:3,c2x4:48")
    ap.add_argument("--beams", default="8,1")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--mti", type=int, default=0, choices=[0, 2, 3])
    a = ap.parse_args()
    import numpy as np
    import torch
    from fmcw import BeamFormer, RadarCore, steering_weights, synth

    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def timed(fn, iters):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return 1e3 * e0.elapsed_time(e1) / iters     # us per call

    for case in a.cases.split(","):
        w, F = case.split(":")
        g, F = GEOM[w], int(F)
        ns, nc, nrx = g["ns"], g["nc"], g["nrx"]
        u = synth.frames(F, ns, nc, nrx, "two_targets", seed=1234).view(np.float32)
        cube = torch.from_numpy(np.ascontiguousarray(u)).to(dev)
        spec = torch.empty((F, nrx, ns, nc, 2), dtype=torch.float32, device=dev)
        with RadarCore(N_RANGE=ns, N_DOPPLER=nc, N_RX=nrx, cfar="none", max_frames=F) as core:
            core.range_ct(cube, spec, F, stream=stream)
            torch.cuda.synchronize()
        del cube
        for nb in (int(x) for x in a.beams.split(",")):
            nus = (np.arange(nb) - nb // 2) / nb
            maps = torch.empty((F, nb, ns, nc), dtype=torch.float32, device=dev)
            with BeamFormer(ns, nc, nrx, steering_weights(nrx, nus), mti=a.mti) as bf:
                us = timed(lambda: bf.enqueue(spec, F, maps, stream=stream), a.iters)
            # a sanity check of what was timed: the first target (range 100 ns / 1024, Doppler 5, a quarter
            # cycle per element) is the peak of its frame in the beam nearest nu = 0.25
            b = int(np.argmin(np.abs(nus - 0.25)))
            peak = int(maps[0, b].argmax().item())
            bytes_ = F * ns * nc * (8 * nrx + 4 * nb)
            print(json.dumps({"case": w, "frames": F, "n_rx": nrx, "n_beams": nb, "mti": a.mti,
                              "beams_us_per_launch": round(us, 1), "compulsory_bytes": bytes_,
                              "compulsory_TBps": round(bytes_ / us / 1e6, 3),
                              "fraction_of_8TBps": round(bytes_ / (us * 1e-6) / HBM_PEAK, 3),
                              "peak_cell_of_beam_at_quarter": [peak // nc, peak % nc] if a.mti == 0 else None}),
                  flush=True)
            del maps
        del spec


if __name__ == "__main__":
    main()
