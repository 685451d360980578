#!/usr/bin/env python3
"""Time the angle resolver (fmcw_doa_enqueue) against fmcw_bearings_enqueue on the same record list.

Per list (sparse: --sparse records, the order of a config-3 detection list; dense: --dense records) and
shape (n_ch, n_grid), for k_max 1 / 2 and relax_passes 0 / 2: the spectrum is white Gaussian on the device
(64 range rows x 128 chirps x n_ch channels; neither stage's time depends on the values), the records are
random cells, fmcw_bearings_enqueue writes the snapshots the resolver then reads.  5 warm-up calls, then
--iters calls each between its own pair of stream events; the figure is the median.  One JSON line per
combination: the median, minimum and maximum per call in us of both stages and the ratio of the medians.
After the timed calls the first 8 records are held to the fp64 specification (tests/doa_ref.py).
usage: python tools/doa_time.py [--iters 30] [--sparse 300] [--dense 65536] [--shapes 16x256,64x1024]"""
import argparse
import json
import statistics
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "fpga-fmcw-radar-processor_amd"))
sys.path.insert(0, str(REPO / "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="16x256,64x1024")
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--sparse", type=int, default=300)
    ap.add_argument("--dense", type=int, default=65536)
    a = ap.parse_args()
    if a.iters < 20:
        ap.error("--iters: the median of at least 20 calls")
    import numpy as np
    import torch
    from fmcw import DOA_DTYPE, AngleResolver, BearingEstimator, line_steering
    import doa_ref as D

    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    nr, nc = 64, 128

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

    def stats(us):
        return {"median": round(statistics.median(us), 1), "min": round(min(us), 1), "max": round(max(us), 1)}

    for shape in a.shapes.split(","):
        nch, ng = (int(x) for x in shape.split("x"))
        gen = torch.Generator(device=dev).manual_seed(1234)
        spec = torch.randn((1, nch, nr, nc, 2), dtype=torch.float32, device=dev, generator=gen) * 1000.0
        steering, _ = line_steering(nch, 0.5, ng)
        for name, n in (("sparse", a.sparse), ("dense", a.dense)):
            rng = np.random.default_rng(n)
            recs = np.zeros((n, 4), np.uint32)                           # fmcw_det: frame, range | doppler << 16, mag, threshold
            recs[:, 1] = rng.integers(0, nr, n) | (rng.integers(0, nc, n) << 16)
            drec = torch.from_numpy(recs.view(np.int32)).to(dev)
            dn = torch.tensor([n], dtype=torch.int32, device=dev)
            bear = torch.empty((n, 8), dtype=torch.int32, device=dev)
            snaps = torch.empty((n, nch, 2), dtype=torch.float32, device=dev)
            out = torch.empty((n, 24), dtype=torch.int32, device=dev)
            st = torch.empty(4, dtype=torch.int32, device=dev)
            with BearingEstimator(nr, nc, nch) as be:
                us_b = timed(lambda: be.enqueue(spec, 1, drec, 16, n, dn, bear, snaps, st, stream=stream))
            for k_max in (1, 2):
                for relax in (0, 2):
                    with AngleResolver(nch, steering, k_max=k_max, relax_passes=relax) as ar:
                        us_d = timed(lambda: ar.enqueue(snaps, bear, 32, n, dn, out, None, st[2:], stream=stream))
                    torch.cuda.synchronize()
                    got = out[:8].cpu().numpy().view(np.uint8).reshape(-1).view(DOA_DTYPE)
                    sn = torch.view_as_complex(snaps[:8]).cpu().numpy()
                    ref = D.resolve_list(sn, steering, k_max=k_max, relax_passes=relax)
                    same = all(list(g["src"]["grid"][: r["n_src"]]) == r["grid"] for g, r in zip(got, ref))
                    line = {"list": name, "records": n, "n_ch": nch, "n_grid": ng, "k_max": k_max, "relax_passes": relax,
                            "doa_us": stats(us_d), "bearings_us": stats(us_b), "calls": a.iters,
                            "doa_over_bearings": round(statistics.median(us_d) / statistics.median(us_b), 2),
                            "first_8_grid_points_as_fp64": bool(same)}
                    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
