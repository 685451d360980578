#!/usr/bin/env python3
"""Time the adaptive beam weights (fmcw_adapt_enqueue) at config 3's shape with 4 and with 16 channels.

The spectrum of a case is complex Gaussian noise drawn on the device (the kernels' time does not depend
on the values); the training window is the whole map.  fmcw_adapt_enqueue is timed with stream events
(3 warm-up calls, then --iters calls between two events), and beside it, in the same run on the same
spectrum, a one-beam fmcw_beams_enqueue: the yardstick, which reads the same bytes.  One JSON line per
case: the mean time per call of each, the compulsory bytes of the covariance pass (8 n_rx per trained
cell: every channel read once) over the adaptive call's time, and that rate as a fraction of the
8 TB/s HBM peak.
usage: python tools/adapt_bench.py [--cases c3:3,c3x16:3] [--iters 20] [--mti 0]
(a case is geometry:frames; c3 = 512 chirps x 4096 samples x 4 rx, c3x16 the same with 16 rx)"""
import argparse
import json
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "fpga-fmcw-radar-processor_amd"))

GEOM = {"c3": dict(ns=4096, nc=512, nrx=4), "c3x16": dict(ns=4096, nc=512, nrx=16),
        "c2x4": dict(ns=1024, nc=256, nrx=4)}
HBM_PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="c3:3,c3x16:3")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--mti", type=int, default=0, choices=[0, 2, 3])
    a = ap.parse_args()
    import numpy as np
    import torch
    from fmcw import AdaptiveWeights, BeamFormer, steering_vectors, steering_weights
    from fmcw.adapt import parse_info

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
        torch.manual_seed(1234)
        spec = torch.randn((F, nrx, ns, nc, 2), dtype=torch.float32, device=dev)
        nus = [0.1]
        wd = torch.empty((1, nrx, 2), dtype=torch.float32, device=dev)
        cov = torch.empty((nrx, nrx, 2), dtype=torch.float64, device=dev)
        info = torch.empty(8, dtype=torch.int32, device=dev)
        maps = torch.empty((F, 1, ns, nc), dtype=torch.float32, device=dev)
        with AdaptiveWeights(ns, nc, nrx, steering_vectors(nrx, nus), loading=1e-2, mti=a.mti) as ad, \
                BeamFormer(ns, nc, nrx, steering_weights(nrx, nus), mti=a.mti) as bf:
            us = timed(lambda: ad.enqueue(spec, F, wd, cov, info, stream=stream), a.iters)
            us_beam = timed(lambda: bf.enqueue(spec, F, maps, stream=stream), a.iters)
        # a sanity check of what was timed: unit gain at the look direction, K, no fallback
        st = parse_info(info.cpu().numpy().view(np.uint32))
        W = wd.cpu().numpy().view(np.complex64).reshape(1, nrx)
        gain = complex((W[0].astype(np.complex128) * steering_vectors(nrx, nus)[0]).sum())
        bytes_ = F * ns * nc * 8 * nrx
        print(json.dumps({"case": w, "frames": F, "n_rx": nrx, "mti": a.mti, "n_units": st["n_units"],
                          "adapt_us_per_call": round(us, 1), "compulsory_bytes": bytes_,
                          "compulsory_TBps": round(bytes_ / us / 1e6, 3),
                          "fraction_of_8TBps": round(bytes_ / (us * 1e-6) / HBM_PEAK, 3),
                          "one_beam_us_per_call": round(us_beam, 1),
                          "adapt_over_one_beam": round(us / us_beam, 3),
                          "K": st["K"], "fallback": st["fallback"], "gain_error": abs(gain - 1.0)}), flush=True)
        del spec, maps


if __name__ == "__main__":
    main()
