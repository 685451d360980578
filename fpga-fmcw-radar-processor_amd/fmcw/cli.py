"""fmcw CLI -- run the MI355X hot path on a file and write the reference's output formats.

    python -m fmcw.cli INPUT [--n-range 1024 --n-doppler 128 --cfar os2d|os1d|ca|go|so|none]
                             [--out-dir DIR] [--quick] [--map-file radar_output.txt]

INPUT formats (by extension):
  .txt   "I Q" integer lines (data/golden_input_chirp.txt); a frame is N_DOPPLER chirps of
         N_RANGE samples; a file shorter than one frame is framed as N_DOPPLER identical
         chirps of its first N_RANGE samples (BASELINE config 1)
  .npy   complex64 [frames][rx][chirp][sample] or [chirp][sample], or int16 [..., 2]
  .bin   raw 32-bit AXI words {Q[31:16], I[15:0]} (radar_core.vhd:25-29), frame-major

Outputs in --out-dir (names the visualizer searches, model/visualize_radar_targets.py:37-107):
  ADR_detections.txt (or ADR_quick_det.txt with --quick): "r d mag" per detection
  radar_output.txt (with --map-file): "r d 0 0 mag" map of the first frame
  --doppler-centred shifts Doppler bins by N/2 (fftshift) in both files
  --cfar ca|go|so [--ca-alpha 4] detects with the cell-averaging family (fmcw.cacfar: CA, greatest-of,
                 smallest-of; the 2-D window 4/1/4/2) on the map of the path run without a CFAR
  --excise zero|interp [--excise-alpha 16 --excise-guard 4] repairs interference bursts in the ADC cube
                 before anything else runs (fmcw.excise: per chirp, samples whose power exceeds alpha x the
                 chirp's median power, widened by the guard, are zeroed or interpolated) and prints the
                 four status words
  ADR_tracks.txt (with --tracks): the track-while-scan log, one scan per frame
                 ("TRK id R= D= Q=" / "SCAN_END ACTIVE=n", tb_radar_core.vhd:163-180);
                 --tracker gpu runs the device tracker (fmcw.tracker_dev) and writes the same file;
                 with --beams B it tracks the beams' detections, one track file per beam
  ADR_plots.txt (with --plots [--plot-window R D]): one line per plot (local-maximum detection
                 of its R x D window, fmcw.plots): "frame r d mag n_cells r+d_range d+d_doppler";
                 with --plots, --tracks feeds the tracker each frame's plots, not its detections
  ADR_bearings.txt (with --bearings [--rx-spacing 0.5]): one line per detection (per plot with
                 --plots): "frame r d power nu sin_theta coherence flags" (fmcw.bearings: the phase
                 step across the receive channels in cycles per element, and nu / spacing)
  ADR_beam_detections.txt (with --beams B [--rx-spacing 0.5]): the channels summed coherently into B
                 beams at nu_b = (b - B/2) / B cycles per element (fmcw.beams), the CFAR run on every
                 beam's map: "frame beam r d mag threshold nu_b sin_theta_b" per detection;
                 with --adaptive LOADING the beams' weights are the minimum-variance ones (fmcw.adapt)
                 trained on the call's own frames over the whole map, for the same look directions
"""
from __future__ import annotations

import argparse
from pathlib import Path

import math

import numpy as np

from . import formats, synth
from .adapt import AdaptiveWeights, steering_vectors
from .beams import BeamFormer, steering_weights
from .cacfar import CaCfar
from .excise import InterferenceExciser
from .bearings import BearingEstimator
from .plots import PlotExtractor
from .radar_core import DET_DTYPE, DeviceBuffer, RadarCore, adc_words_to_cube
from .tracker import TwsTracker
from .tracker_dev import DeviceTwsTracker


def load_cube(path: Path, ns: int, nc: int):
    if path.suffix == ".txt":
        iq = formats.read_adc_pairs(path)
        per = ns * nc
        if len(iq) < per:
            return synth.golden_chirp_frame(iq, nc, ns)[None], "f32"
        nf = len(iq) // per
        z = (iq[: nf * per, 0] + 1j * iq[: nf * per, 1]).astype(np.complex64)
        return z.reshape(nf, 1, nc, ns), "f32"
    if path.suffix == ".npy":
        a = np.load(path, allow_pickle=False)
        if a.dtype == np.int16:
            return a.reshape(-1, 1, nc, ns, 2) if a.ndim <= 4 else a, "i16"
        a = a.astype(np.complex64)
        return a.reshape(-1, 1, nc, ns) if a.ndim <= 3 else a, "f32"
    if path.suffix == ".bin":
        w = np.fromfile(path, dtype="<u4")
        nf = len(w) // (ns * nc)
        return adc_words_to_cube(w[: nf * ns * nc].reshape(nf, nc * ns), nc, ns).reshape(nf, 1, nc, ns, 2), "i16"
    raise SystemExit(f"unsupported input {path}")


def build_parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("input", type=Path)
    ap.add_argument("--n-range", type=int, default=1024)
    ap.add_argument("--n-doppler", type=int, default=128)
    ap.add_argument("--cfar", default="os2d", choices=["os2d", "os1d", "ca", "go", "so", "none"])
    ap.add_argument("--ca-alpha", type=float, default=4.0, metavar="ALPHA",
                    help="threshold factor of --cfar ca / go / so (finite, > 0)")
    ap.add_argument("--out-dir", type=Path, default=Path("."))
    ap.add_argument("--quick", action="store_true", help="write ADR_quick_det.txt (128x32 geometry)")
    ap.add_argument("--map-file", default=None)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--tracks", action="store_true", help="run the TWS tracker, write ADR_tracks.txt")
    ap.add_argument("--tracker-rtl", action="store_true", help="tracker in RTL-compat mode")
    ap.add_argument("--tracker", default="host", choices=["host", "gpu"],
                    help="with --tracks: the host tracker, one frame at a time (default), or the device "
                         "tracker over the whole call's list (with --beams B: one track file per beam)")
    ap.add_argument("--plots", action="store_true",
                    help="group the detections into plots (one per local maximum), write ADR_plots.txt; "
                         "--tracks then tracks the plots")
    ap.add_argument("--plot-window", type=int, nargs=2, default=[1, 1], metavar=("R", "D"),
                    help="plot window half-widths in range and Doppler bins (0..4 each)")
    ap.add_argument("--window", default="hamming", choices=["hamming", "none", "q15_rtl"])
    ap.add_argument("--doppler-centred", action="store_true",
                    help="write Doppler bins fftshifted (zero Doppler at N/2, as the visualizer assumes)")
    ap.add_argument("--bearings", action="store_true",
                    help="estimate the bearing of every detection (of every plot with --plots) from the "
                         "phase across the receive channels, write ADR_bearings.txt")
    ap.add_argument("--rx-spacing", type=float, default=0.5, metavar="WAVELENGTHS",
                    help="element spacing of the receive array in wavelengths (with --bearings, --beams)")
    ap.add_argument("--beams", type=int, default=0, metavar="B",
                    help="sum the receive channels coherently into B beams (1..64) at (b - B/2) / B cycles per "
                         "element, run the CFAR on every beam's map, write ADR_beam_detections.txt")
    ap.add_argument("--adaptive", type=float, default=None, metavar="LOADING",
                    help="with --beams: adaptive (MVDR) weights for the same look directions, trained on the "
                         "call's frames, diagonal loading LOADING (finite, >= 0) of the mean channel power")
    ap.add_argument("--excise", default=None, choices=["zero", "interp"],
                    help="repair interference bursts in the ADC cube first: zero them, or interpolate across them")
    ap.add_argument("--excise-alpha", type=float, default=16.0, metavar="ALPHA",
                    help="with --excise: flag samples whose power exceeds ALPHA x the chirp's median (finite, >= 1)")
    ap.add_argument("--excise-guard", type=int, default=4, metavar="SAMPLES",
                    help="with --excise: samples repaired on each side of a flagged one (0..32)")
    return ap


CA_MODES = ("ca", "go", "so")


def beam_detections(core_args: dict, spec, nf: int, nrx: int, n_beams: int, window: str, device: int,
                    ca_alpha: float = 4.0, adaptive: float | None = None):
    """The CFAR of `core_args` over the n_frames * n_beams beamformed maps of the device spectrum
    `spec`: (detections with frame = f * n_beams + b, the beams' nu).  adaptive: the loading of
    AdaptiveWeights, whose weights then replace the steering weights before the beams are formed."""
    ns, nc = core_args["N_RANGE"], core_args["N_DOPPLER"]
    nus = (np.arange(n_beams) - n_beams // 2) / n_beams
    n_maps = nf * n_beams
    maps = DeviceBuffer(n_maps * ns * nc * 4, device)
    with BeamFormer(ns, nc, nrx, steering_weights(nrx, nus), window=window, device=device) as bf:
        if adaptive is not None:
            with AdaptiveWeights(ns, nc, nrx, steering_vectors(nrx, nus), loading=adaptive, device=device) as ad:
                dw, di = DeviceBuffer(ad.w_bytes(), device), DeviceBuffer(32, device)
                ad.enqueue(spec, nf, dw, None, di)
                bf.set_weights_dev(dw)
                bf.enqueue(spec, nf, maps)
                if int(di.download(np.uint32, (8,))[2]) & 1:
                    print("adaptive weights: the covariance could not be factorised, conventional beams used")
                dw.free()
                di.free()
        else:
            bf.enqueue(spec, nf, maps)
    if core_args["cfar"] in CA_MODES:
        with CaCfar(ns, nc, mode=core_args["cfar"], alpha=ca_alpha, max_frames=n_maps, device=device) as ca:
            dets = ca.detect(maps)
        maps.free()
        return dets, nus
    dn = DeviceBuffer(16, device)
    with RadarCore(N_RX=1, max_frames=n_maps, **core_args) as core:   # the CFAR stage alone: it sees maps only
        cap = n_maps * 4096
        while True:
            dd = DeviceBuffer(cap * DET_DTYPE.itemsize, device)
            core.cfar(maps, n_maps, dd, cap, dn)
            found = int(dn.download(np.uint32, (4,))[0])
            if found <= cap:
                dets = dd.download(DET_DTYPE, (found,))
                dd.free()
                break
            dd.free()
            cap = found
    maps.free()
    dn.free()
    return dets, nus


def main(argv=None):
    ap = build_parser()
    a = ap.parse_args(argv)
    if a.bearings and a.window == "q15_rtl":
        ap.error("--bearings needs a float window (hamming or none)")
    if (a.bearings or a.beams) and not a.rx_spacing > 0:
        ap.error("--rx-spacing must be positive")
    if a.beams and a.window == "q15_rtl":
        ap.error("--beams needs a float window (hamming or none)")
    if a.beams and not 1 <= a.beams <= 64:
        ap.error("--beams must be in 1..64")
    if a.adaptive is not None and not a.beams:
        ap.error("--adaptive needs --beams")
    if a.adaptive is not None and not (math.isfinite(a.adaptive) and a.adaptive >= 0):
        ap.error("--adaptive LOADING must be finite and >= 0")
    if a.beams and a.cfar == "none":
        ap.error("--beams needs a CFAR (os1d or os2d) to run on the beams' maps")
    if not (math.isfinite(a.ca_alpha) and a.ca_alpha > 0):
        ap.error("--ca-alpha must be finite and positive")
    if not (math.isfinite(a.excise_alpha) and a.excise_alpha >= 1):
        ap.error("--excise-alpha must be finite and >= 1")
    if not 0 <= a.excise_guard <= 32:
        ap.error("--excise-guard must be in 0..32")
    ca = a.cfar in CA_MODES
    cube, dt = load_cube(a.input, a.n_range, a.n_doppler)
    nf, nrx = cube.shape[0], cube.shape[1]
    if a.excise:   # the interference exciser on the cube, in front of everything else
        with InterferenceExciser(a.n_range, a.n_doppler, n_rx=nrx, in_dtype=dt, mode=a.excise, guard=a.excise_guard,
                                 alpha=a.excise_alpha, max_frames=nf, device=a.device) as ex:
            cube, _, _, st = ex.repair(np.ascontiguousarray(cube))
        print(f"excise {a.excise}: {st[0]} samples repaired in {st[1]} chirps ({st[2]} flagged before the guard, "
              f"{st[3]} chirps more than half repaired)")
    if a.beams and nrx < 2:
        ap.error(f"--beams needs multi-rx input ({a.input} has one channel)")
    if a.adaptive is not None and nrx > 16:
        ap.error(f"--adaptive takes at most 16 channels ({a.input} has {nrx})")
    spec = None
    with RadarCore(N_RANGE=a.n_range, N_DOPPLER=a.n_doppler, N_RX=nrx, in_dtype=dt,
                   cfar="none" if ca else a.cfar, max_frames=nf, device=a.device, window=a.window) as core:
        cube = np.ascontiguousarray(cube)
        out = core.process(cube)
        if a.bearings or a.beams:   # the corner-turned spectrum still carries the channels' phases
            dc = DeviceBuffer(cube.nbytes, a.device)
            dc.upload(cube)
            spec = DeviceBuffer(nf * nrx * a.n_range * a.n_doppler * 8, a.device)
            core.range_ct(dc, spec, nf)
            dc.free()
    dets = out.dets
    if ca:   # the cell-averaging detector on the path's map
        with CaCfar(a.n_range, a.n_doppler, mode=a.cfar, alpha=a.ca_alpha, max_frames=nf, device=a.device) as det:
            dets = det.detect(out.rd_map)
    a.out_dir.mkdir(parents=True, exist_ok=True)
    det_name = "ADR_quick_det.txt" if a.quick else "ADR_detections.txt"
    n = formats.write_detections(a.out_dir / det_name, dets, doppler_centred=a.doppler_centred,
                                 n_doppler=a.n_doppler)
    if a.map_file:
        formats.write_rd_map(a.out_dir / a.map_file, out.rd_map[0], doppler_centred=a.doppler_centred)
    print(f"{nf} frame(s) {a.n_doppler}x{a.n_range}: {n} detections -> {a.out_dir / det_name}")
    scans = dets
    if a.plots:
        with PlotExtractor(N_RANGE=a.n_range, N_DOPPLER=a.n_doppler, win=tuple(a.plot_window),
                           max_dets=max(len(dets), 1), device=a.device) as px:
            scans = px.extract(dets)
        formats.write_plots(a.out_dir / "ADR_plots.txt", scans, doppler_centred=a.doppler_centred,
                            n_doppler=a.n_doppler)
        print(f"{len(scans)} plots (window {a.plot_window[0]} x {a.plot_window[1]}) -> {a.out_dir / 'ADR_plots.txt'}")
    if a.bearings:
        with BearingEstimator(N_RANGE=a.n_range, N_DOPPLER=a.n_doppler, N_RX=nrx, window=a.window,
                              spacing=a.rx_spacing, max_records=max(len(scans), 1), device=a.device) as be:
            bearings, _ = be.estimate(spec, scans, want_snaps=False)
        formats.write_bearings(a.out_dir / "ADR_bearings.txt", bearings, doppler_centred=a.doppler_centred,
                               n_doppler=a.n_doppler)
        print(f"{len(bearings)} bearings ({nrx} rx, spacing {a.rx_spacing}) -> {a.out_dir / 'ADR_bearings.txt'}")
    if a.beams:
        bdets, nus = beam_detections(dict(N_RANGE=a.n_range, N_DOPPLER=a.n_doppler, cfar=a.cfar, device=a.device),
                                     spec, nf, nrx, a.beams, a.window, a.device, a.ca_alpha, a.adaptive)
        formats.write_beam_detections(a.out_dir / "ADR_beam_detections.txt", bdets, nus, spacing=a.rx_spacing,
                                      doppler_centred=a.doppler_centred, n_doppler=a.n_doppler)
        print(f"{len(bdets)} detections in {a.beams} beams ({nrx} rx, spacing {a.rx_spacing}) -> "
              f"{a.out_dir / 'ADR_beam_detections.txt'}")
    if spec is not None:
        spec.free()
    if a.tracks and a.tracker == "gpu":
        # the whole call's list through the device tracker; with --beams, one track file per beam
        # over the beams' detections (frame = f * B + b), grouped into plots first with --plots
        n_streams, recs = 1, scans
        if a.beams:
            n_streams, recs = a.beams, bdets
            if a.plots:
                with PlotExtractor(N_RANGE=a.n_range, N_DOPPLER=a.n_doppler, win=tuple(a.plot_window),
                                   max_dets=max(len(bdets), 1), device=a.device) as px:
                    recs = px.extract(bdets)
        with DeviceTwsTracker(n_streams=n_streams, max_scans=nf, device=a.device,
                              rtl_compat=a.tracker_rtl) as trk:
            formats.write_tracks(a.out_dir / "ADR_tracks.txt", trk.run(recs, nf))
    elif a.tracks:
        with TwsTracker(rtl_compat=a.tracker_rtl) as trk:
            hist = []
            for f in range(nf):
                tracks = trk.scan(scans[scans["frame"] == f])
                hist.append((tracks, trk.active_tracks))
        formats.write_tracks(a.out_dir / "ADR_tracks.txt", hist)


if __name__ == "__main__":
    main()
