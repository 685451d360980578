#!/usr/bin/env python3
"""Time the TDM-MIMO virtual array (fmcw_mimo_enqueue) at three shapes.

Per shape and alignment mode: the spectrum is built once (white Gaussian on the device; the stage's time
does not depend on the values), 5 warm-up launches, then --iters launches each between its own pair of
stream events; the figure is the median.  One JSON line per (shape, mode): the median, minimum and maximum
time per launch in us, the compulsory bytes (16 B per point: every point read once and written once)
over the median, and that rate as a fraction of the float4-copy ceiling of DESIGN.md section 3
(6.29 TB/s).  ALIGN_NONE is the pure-traffic floor of the same launch; the last field of a "dft" line is
its time over that floor.  After the timed launches "dft" is held to the fp64 specification on one row of
each channel of the last frame (the row's error over 1e-4 of its maximum), "none" to the input's bytes on
the same rows.
usage: python tools/mimo_time.py [--iters 30] [--shapes 4096x512x4x3:2,8192x1024x1x3:4,1024x256x1x104:2]
(a shape is n_range x n_chirps x n_rx x frames : n_tx)"""
import argparse
import json
import statistics
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "fpga-fmcw-radar-processor_amd"))
sys.path.insert(0, str(REPO / "tests"))

COPY_CEILING = 6.29e12      # B/s: the float4 copy of DESIGN.md section 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="4096x512x4x3:2,8192x1024x1x3:4,1024x256x1x104:2")
    ap.add_argument("--iters", type=int, default=30)
    a = ap.parse_args()
    if a.iters < 20:
        ap.error("--iters: the median of at least 20 launches")
    import numpy as np
    import torch
    from fmcw import VirtualArray
    import mimo_ref as M

    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def timed(fn):
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        us = []
        for _ in range(a.iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            us.append(1e3 * e0.elapsed_time(e1))
        return us

    for shape in a.shapes.split(","):
        dims, ntx = shape.split(":")
        ns, nc, nrx, F = (int(x) for x in dims.split("x"))
        ntx = int(ntx)
        gen = torch.Generator(device=dev).manual_seed(1234)
        spec = torch.randn((F, nrx, ns, nc, 2), dtype=torch.float32, device=dev, generator=gen) * 1000.0
        out = torch.empty_like(spec)
        points = F * nrx * ns * nc
        floor = None
        for align in ("none", "dft"):
            out.fill_(0)
            with VirtualArray(ns, nc, nrx, ntx, align=align) as va:
                us = timed(lambda: va.enqueue(spec, F, out, stream=stream))
            torch.cuda.synchronize()
            # what was timed, on row r = 5 of every channel of the last frame
            r = 5
            x = torch.view_as_complex(spec[F - 1, :, r]).cpu().numpy()[None, :, None, :]
            got = torch.view_as_complex(out.view(F, ntx * nrx, ns, nc // ntx, 2)[F - 1, :, r]).cpu().numpy()[None, :, None, :]
            if align == "dft":
                check = round(M.bound_used(got, M.mimo_ref(x, ntx)), 4)
            else:
                check = bool(got.tobytes() == M.mimo_ref(x, ntx, "none").tobytes())
            med = statistics.median(us)
            line = {"n_range": ns, "n_chirps": nc, "n_rx": nrx, "frames": F, "n_tx": ntx, "align": align,
                    "us_median": round(med, 1), "us_min": round(min(us), 1), "us_max": round(max(us), 1),
                    "launches": len(us), "bytes": 16 * points, "TBps": round(16 * points / med / 1e6, 3),
                    "of_copy_ceiling": round(16 * points / (med * 1e-6) / COPY_CEILING, 3),
                    "bound_used" if align == "dft" else "bytes_equal": check}
            if align == "none":
                floor = med
            else:
                line["over_none"] = round(med / floor, 2)
            print(json.dumps(line), flush=True)
        del spec, out


if __name__ == "__main__":
    main()
