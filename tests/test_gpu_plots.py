"""Plot extraction on the GPU (fmcw_plots_* of libfmcw.so on gfx950 through the C-ABI), every case
against tests/plots_ref.py (the specification in NumPy, fp64 sums) run on the same list.

Tolerances (plots_ref.assert_plots_match): frame / range / doppler / mag / threshold / n_cells, the
order and the count exact; sum_mag within 1e-5 relative (<= 81 positive fp32 terms, <= 80 * 2^-24
= 4.8e-6 in any order); d_range / d_doppler within 1e-4 bins (81 * 2^-24 * 4 for the numerator
plus 4 * 4.8e-6 for the division, about 4e-5).
"""
import functools

import numpy as np
import pytest

import reclist_cases as RC
from conftest import GOLDEN
from fmcw import (RadarCore, BeamMerger, DeviceBuffer, DET_DTYPE, PLOT_DTYPE, PlotExtractor, TwsTracker, formats,
                  synth)
from plots_ref import plots_ref, assert_plots_match
from gpu_support import SENTINEL, Hip, cli, run_rec_list

pytestmark = pytest.mark.gpu


def mk(rows):
    """DET_DTYPE list from (frame, range, doppler, mag) rows (sorted here), threshold = mag / 2."""
    a = np.zeros(len(rows), DET_DTYPE)
    for i, (f, r, d, m) in enumerate(sorted(rows)):
        a[i] = (f, r, d, m, 0.5 * m)
    return a


def random_list(seed, nf, nr, nd, density, levels=5):
    rng = np.random.default_rng(seed)
    f, r, d = np.nonzero(rng.random((nf, nr, nd)) < density)
    a = np.zeros(len(f), DET_DTYPE)
    a["frame"], a["range"], a["doppler"] = f, r, d
    a["mag"] = rng.integers(1, levels + 1, len(f)).astype(np.float32)
    a["threshold"] = rng.random(len(f)).astype(np.float32)
    return a


def run(px, dets, plot_cap=None, det_cap=None, n_word=None):
    """One fmcw_plots_enqueue on a host list: (status words, plots written, the sentinel-filled plot
    buffer's bytes after them).  The two status words sit between guard words."""
    def enqueue(dd, stride, det_cap, dn, dp, plot_cap, ds):
        px.enqueue(dd, det_cap, dn, dp, plot_cap, ds)
    plot_cap = max(len(dets), 1) if plot_cap is None else plot_cap
    return run_rec_list(enqueue, dets, PLOT_DTYPE, 2, plot_cap, det_cap, n_word, guards=(4, 2))


def check(dets, nr, nd, win, **kw):
    want = plots_ref(dets, nr, nd, *win)
    with PlotExtractor(nr, nd, win=win, max_dets=max(len(dets), 1)) as px:
        st, got, rest = run(px, dets, **kw)
    assert list(st) == [len(want), 0], st
    assert_plots_match(got, want)
    assert np.all(rest == SENTINEL)
    return got


HAND = {
    "doppler_wrap": ([(0, 3, 0, 2.0), (0, 3, 7, 5.0), (0, 4, 0, 1.0), (0, 5, 7, 9.0), (0, 5, 1, 8.0)], (1, 1)),
    "range_clamp": ([(0, 0, 2, 1.0), (0, 7, 2, 3.0), (0, 0, 3, 2.0), (0, 7, 3, 1.0), (0, 1, 2, 7.0), (0, 6, 3, 4.0)],
                    (1, 1)),
    "adjacent_frames": ([(0, 7, 7, 3.0), (1, 0, 0, 4.0), (1, 7, 7, 5.0), (2, 7, 7, 1.0), (2, 0, 0, 2.0)], (1, 1)),
    "plateau_2x2": ([(0, 2, 2, 4.0), (0, 2, 3, 4.0), (0, 3, 2, 4.0), (0, 3, 3, 4.0), (0, 4, 4, 1.0)], (1, 1)),
    "plateau_row": ([(0, 4, d, 6.0) for d in range(8)] + [(1, 4, d, 6.0) for d in range(1, 7)], (1, 1)),
    "win_0_0": ([(0, r, d, float(1 + (r * d) % 3)) for r in range(8) for d in range(0, 8, 2)], (0, 0)),
}


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_made_8x8(gpu, name):
    """Doppler wrap (columns 7 and 0 are neighbours), clamping at range 0 and 7, the same cell in
    adjacent frames (no grouping), a 2 x 2 plateau (first in list order wins), plateau rows longer
    than the window (a whole circular row and a run inside a row: by the tie rule each gives one
    peak, its first cell), window (0, 0) (one plot per detection, n_cells 1)."""
    rows, win = HAND[name]
    dets = mk(rows)
    got = check(dets, 8, 8, win)
    if name == "win_0_0":
        assert len(got) == len(dets) and np.all(got["n_cells"] == 1)
    if name == "plateau_2x2":
        assert (int(got["range"][0]), int(got["doppler"][0]), int(got["n_cells"][0])) == (2, 2, 4)
    if name == "plateau_row":
        # every cell but a run's first has an equal neighbour before it in the list: one peak per
        # run, at its first cell (frame 0: the whole circular row; frame 1: columns 1..6)
        assert [(int(p["frame"]), int(p["doppler"]), int(p["n_cells"])) for p in got] == [(0, 0, 3), (1, 1, 2)]
    if name == "adjacent_frames":
        assert len(got) == len(dets)


def test_win_4_4_n_doppler_9(gpu):
    """The widest window on the narrowest map it fits: every row of the window is the whole
    (circular) Doppler axis."""
    check(random_list(5, 2, 8, 9, 0.6), 8, 9, (4, 4))


@pytest.mark.parametrize("win", [(1, 1), (2, 1), (1, 2), (0, 3), (4, 4)])
def test_random_lists(gpu, win):
    """3 frames x 64 x 32 at density 0.3, magnitudes from {1..5} so that ties are everywhere."""
    check(random_list(11, 3, 64, 32, 0.3), 64, 32, win)


@pytest.mark.parametrize("density", [0.5, 1.0])
def test_larger_lists(gpu, density):
    """2 frames x 256 x 128: the list spans many workgroup tiles, frame and row boundaries fall
    inside a tile, and at density 1.0 a window row lies beyond the staged neighbourhood."""
    dets = random_list(12, 2, 256, 128, density)
    check(dets, 256, 128, (1, 1))
    check(dets, 256, 128, (4, 4))


@pytest.mark.parametrize("nf,nr,nd,density,win,grids", [(3, 16, 9, 0.5, (1, 1), (0,)), (3, 16, 9, 0.5, (4, 4), (0,)),
                                                         (2, 64, 32, 1.0, (4, 4), (0, 1))])
def test_equals_the_merger_on_one_beam(gpu, nf, nr, nd, density, win, grids):
    """The plot extractor and the beam merger with one beam and win_beam 0 run the same walk, so on the
    same ordered list their records agree bit for bit.  16 x 9: n_doppler = 2 * 4 + 1, the window wraps
    on both sides at every cell.  64 x 32 x 2 at density 1: 4096 records, 4 tiles with halos on both
    sides, under the built-in grid and under one workgroup."""
    dets = random_list(71, nf, nr, nd, density)
    assert density < 1.0 or len(dets) == 4096
    with PlotExtractor(nr, nd, win=win, max_dets=len(dets)) as px, \
            BeamMerger(nr, nd, 1, win=(0, *win), max_recs=len(dets), max_maps=nf) as mg:
        for grid in grids:
            px.set_grid_for_test(grid)
            mg.set_grid_for_test(grid)
            p, m = px.extract(dets), mg.merge(dets, nf)
            assert len(p) == len(m) > 0
            for name in ("frame", "range", "doppler", "mag", "sum_mag", "d_range", "d_doppler"):
                assert p[name].tobytes() == m[name].tobytes(), (grid, name)
            assert np.array_equal(p["n_cells"], m["n_merged"])
            assert not m["d_beam"].any() and not m["beam"].any()


def test_corner_list_at_the_limits(gpu):
    """n_range = n_doppler = 65536, records at the four corners and their neighbours across the Doppler wrap,
    window (4, 4) (reclist_cases.py; the list layer ran the same list on the CPU under sanitizers,
    test_reclist_replay.py).  max_dets is the list's length; one workgroup and the built-in grid, the same bytes."""
    dets = RC.corner_list(3, DET_DTYPE)
    want = plots_ref(dets, RC.LIMIT, RC.LIMIT, *RC.PLOTS_CORNER_WIN)
    assert 0 < len(want) < len(dets) and want["n_cells"].max() > 4
    first = None
    with PlotExtractor(RC.LIMIT, RC.LIMIT, win=RC.PLOTS_CORNER_WIN, max_dets=len(dets)) as px:
        for grid in (1, 0):
            px.set_grid_for_test(grid)
            st, got, rest = run(px, dets)
            assert list(st) == [len(want), 0], (grid, st)
            assert_plots_match(got, want)
            assert np.all(rest == SENTINEL), grid
            first = first or (got.tobytes(), rest.tobytes())
            assert (got.tobytes(), rest.tobytes()) == first, grid


def test_empty_list(gpu):
    with PlotExtractor(64, 32) as px:
        st, got, rest = run(px, np.zeros(0, DET_DTYPE), plot_cap=8)
    assert list(st) == [0, 0] and len(got) == 0 and np.all(rest == SENTINEL)


def test_plot_cap_shorter_than_count(gpu):
    dets = random_list(13, 3, 64, 32, 0.3)
    want = plots_ref(dets, 64, 32, 1, 1)
    cap = len(want) // 3
    with PlotExtractor(64, 32, max_dets=len(dets)) as px:
        st, got, rest = run(px, dets, plot_cap=cap)
        assert list(st) == [len(want), 0]
        assert_plots_match(got, want[:cap])
        assert np.all(rest == SENTINEL)
        # extract() retries once with the reported count
        assert_plots_match(px.extract(dets, plot_cap=cap), want)


@functools.lru_cache(maxsize=None)
def _larger(win):
    dets = random_list(12, 2, 256, 128, 0.5)
    want = plots_ref(dets, 256, 128, *win)
    for a in (dets, want):
        a.setflags(write=False)
    return dets, want


@pytest.mark.parametrize("win", [(1, 1), (4, 4)])
def test_capped_grid_larger_list(gpu, win):
    """k_plots_find and k_plots_emit stride over the 1024-record tiles with up to 4096 workgroups, so a
    workgroup takes a second tile only beyond 4.2 M records.  test_larger_lists' list (about 32 tiles)
    under 1 and 3 workgroups (fmcw_plots_set_grid_for_test: every tile after another on the same
    staging arrays; 3 does not divide the tile count): the reference's plots, and the same bytes as
    under the built-in grid, the sentinel beyond the plots included."""
    dets, want = _larger(win)
    assert len(dets) > 30 * 1024
    with PlotExtractor(256, 128, win=win, max_dets=len(dets)) as px:
        st0, got0, rest0 = run(px, dets)
        assert list(st0) == [len(want), 0]
        assert_plots_match(got0, want)
        for grid in (1, 3, 0):
            px.set_grid_for_test(grid)
            st, got, rest = run(px, dets)
            assert list(st) == [len(want), 0], grid
            assert_plots_match(got, want)
            assert got.tobytes() == got0.tobytes() and rest.tobytes() == rest0.tobytes(), grid
            assert np.all(rest == SENTINEL)


def test_capped_grid_plot_cap_shorter_than_count(gpu):
    """test_plot_cap_shorter_than_count's list (two tiles) under 1 and 3 workgroups: the first
    plot_cap plots, nothing stored beyond them (a later tile's offset is past plot_cap: k_plots_emit
    leaves its loop), byte for byte what the built-in grid writes."""
    dets = random_list(13, 3, 64, 32, 0.3)
    want = plots_ref(dets, 64, 32, 1, 1)
    assert len(dets) > 1024
    cap = len(want) // 3
    with PlotExtractor(64, 32, max_dets=len(dets)) as px:
        st0, got0, rest0 = run(px, dets, plot_cap=cap)
        for grid in (1, 3):
            px.set_grid_for_test(grid)
            st, got, rest = run(px, dets, plot_cap=cap)
            assert list(st) == [len(want), 0] == list(st0)
            assert_plots_match(got, want[:cap])
            assert np.all(rest == SENTINEL)
            assert got.tobytes() == got0.tobytes() and rest.tobytes() == rest0.tobytes()
            assert_plots_match(px.extract(dets, plot_cap=cap), want)


def scan_rounds_list():
    """The first 1024 * 1024 + 1 cells (1025 tiles) of 20 frames of 1024 x 128 filled at a density that
    changes with the frame (0.30 .. 0.65), in (frame, range, doppler) order, no cell twice.  Magnitudes
    from {1..5} (the last record: 9): ties everywhere, the peak counts differ from tile to tile, and
    every sum of at most 9 of them, times an offset of at most 1, is exact in fp32 in any order."""
    nf, nr, nd, n = 20, 1024, 128, 1024 * 1024 + 1
    rng = np.random.default_rng(71)
    density = 0.30 + 0.05 * (np.arange(nf) % 8)
    f, r, d = np.nonzero(rng.random((nf, nr, nd)) < density[:, None, None])
    assert len(f) >= n
    a = np.zeros(n, DET_DTYPE)
    a["frame"], a["range"], a["doppler"] = f[:n], r[:n], d[:n]
    a["mag"] = rng.integers(1, 6, n).astype(np.float32)
    a["mag"][-1] = 9.0             # the one record of tile 1024 is a peak
    a["threshold"] = rng.random(n).astype(np.float32)
    return a, nr, nd


def test_scan_beyond_its_first_round(gpu):
    """1025 tiles: k_plots_scan (det_sink.hpp tile_offsets_scan, in place on the tile counts) takes a
    second round of 1024 tiles, and tile 1024's offset is the first round's total.  Unequal, non-zero
    peak counts per tile: a wrong carry or offset moves plots.  The built-in grid, and 3 workgroups,
    each reading offsets of both rounds.  With this list's small integer magnitudes the fp32 sums are
    exact and d_range / d_doppler are one correctly rounded division, so beyond assert_plots_match
    every field equals the reference's rounded to fp32."""
    dets, nr, nd = scan_rounds_list()
    n = len(dets)
    want = plots_ref(dets, nr, nd, 1, 1)
    key = lambda a: (a["frame"].astype(np.int64) * nr + a["range"]) * nd + a["doppler"]
    per_tile = np.bincount(np.searchsorted(key(dets), key(want)) // 1024, minlength=1025)
    assert len(per_tile) == 1025 and per_tile.min() >= 1 and len(set(per_tile.tolist())) > 1
    with PlotExtractor(nr, nd, win=(1, 1), max_dets=n) as px:
        for grid in (0, 3):
            px.set_grid_for_test(grid)
            st, got, rest = run(px, dets, plot_cap=len(want) + 4)
            assert list(st) == [len(want), 0], grid
            assert_plots_match(got, want)
            for name in ("sum_mag", "d_range", "d_doppler"):
                np.testing.assert_array_equal(got[name], want[name].astype(np.float32), err_msg=f"{name}, grid {grid}")
            assert np.all(rest == SENTINEL)


def test_truncated_input(gpu):
    """n_dets_dev[0] above det_cap, and above max_dets: the first n records are examined, word [1]
    counts the rest, and the plots equal the reference on the truncated list."""
    dets = random_list(14, 3, 64, 32, 0.3)
    n = len(dets)
    with PlotExtractor(64, 32, max_dets=n) as px:                 # det_cap binds
        cap = n - 700
        st, got, rest = run(px, dets, det_cap=cap, n_word=n + 5)
    want = plots_ref(dets[:cap], 64, 32, 1, 1)
    assert list(st) == [len(want), n + 5 - cap]
    assert_plots_match(got, want)
    assert np.all(rest == SENTINEL)
    md = 1500
    with PlotExtractor(64, 32, max_dets=md) as px:                # max_dets binds
        st, got, rest = run(px, dets, det_cap=n, n_word=n)
    want = plots_ref(dets[:md], 64, 32, 1, 1)
    assert list(st) == [len(want), n - md]
    assert_plots_match(got, want)
    assert np.all(rest == SENTINEL)


def test_graph_capture_after_enqueue(gpu):
    """fmcw_enqueue (2-D CFAR, 256 x 64, 2 frames) and fmcw_plots_enqueue captured in one graph on
    one stream, replayed on two different cubes (and the first again)."""
    ns, nc, nf = 256, 64, 2
    cubes = [np.ascontiguousarray(synth.frames(nf, ns, nc, 1, "two_targets", seed=71)),
             np.ascontiguousarray(synth.frames(nf, ns, nc, 1, "random_target", seed=72))]
    hip = Hip()
    cap, pcap = nf * ns * nc, 4096
    with RadarCore(N_RANGE=ns, N_DOPPLER=nc, cfar="os2d", max_frames=nf) as core, \
            PlotExtractor(ns, nc, win=(1, 1), max_dets=cap) as px:
        dc = DeviceBuffer(cubes[0].nbytes)
        dd, dn = DeviceBuffer(cap * 16), DeviceBuffer(16)
        dp, ds = DeviceBuffer(pcap * 32), DeviceBuffer(8)

        def both(s):
            core.enqueue(dc, nf, None, dd, cap, dn, stream=s.value)
            px.enqueue(dd, cap, dn, dp, pcap, ds, stream=s.value)
        with hip.graph(both) as (exe, s):
            counts = []
            for k in (0, 1, 0):
                dc.upload(cubes[k])
                hip.replay(exe, s)
                n = int(dn.download(np.uint32, (4,))[0])
                dets = dd.download(DET_DTYPE, (n,))
                want = plots_ref(dets, ns, nc, 1, 1)
                st = ds.download(np.uint32, (2,))
                assert n > 0 and list(st) == [len(want), 0], (k, n, st)
                assert_plots_match(dp.download(PLOT_DTYPE, (len(want),)), want)
                counts.append(dets.tobytes())
            assert counts[0] == counts[2] and counts[0] != counts[1]   # the replays saw their own cubes


def _firm_near(tracks, r, d, nd, gate_r=10, gate_d=5):
    out = []
    for t in tracks:
        dr = abs(int(t["range_q2"]) / 4 - r)
        dv = abs(int(t["doppler_q2"]) / 4 - d)
        if t["status"] == 2 and dr <= gate_r and min(dv, nd - dv) <= gate_d:
            out.append(t)
    return out


def test_end_to_end_tracker(gpu):
    """RadarCore(1024, 128) on 4 frames of two_targets: the plots equal the reference on the GPU's
    own detections, and fed frame by frame to TwsTracker they give a FIRM track within the
    association gate of (500, 118); the raw detections give none there (the tracker's 64 slots go
    to the target at range 100)."""
    ns, nc, nf = 1024, 128, 4
    cube = synth.frames(nf, ns, nc, 1, "two_targets", seed=1234)
    with RadarCore(N_RANGE=ns, N_DOPPLER=nc, max_frames=nf) as core:
        out = core.process(cube)
    with PlotExtractor(ns, nc, win=(1, 1)) as px:
        plots = px.extract(out.dets)
    assert_plots_match(plots, plots_ref(out.dets, ns, nc, 1, 1))
    assert len(plots) < len(out.dets) // 8
    firm = {}
    for name, scans in (("plots", plots), ("dets", out.dets)):
        with TwsTracker() as trk:
            for f in range(nf):
                tracks = trk.scan(scans[scans["frame"] == f])
        firm[name] = _firm_near(tracks, 500, 118, nc)
    assert len(firm["plots"]) >= 1 and len(firm["dets"]) == 0, firm


def test_cli_plots(gpu, tmp_path):
    """--plots --tracks on the golden chirp writes ADR_plots.txt (the reference on the run's own
    detections); without --plots the files are the same as before (no ADR_plots.txt, the same
    detection and track files)."""
    common = (GOLDEN / "golden_input_chirp.txt", "--n-range", 256, "--n-doppler", 128, "--cfar", "os1d", "--tracks")
    a, b = tmp_path / "plain", tmp_path / "plots"
    cli(*common, "--out-dir", a)
    cli(*common, "--out-dir", b, "--plots", "--plot-window", 1, 2)
    assert sorted(p.name for p in a.iterdir()) == ["ADR_detections.txt", "ADR_tracks.txt"]
    assert sorted(p.name for p in b.iterdir()) == ["ADR_detections.txt", "ADR_plots.txt", "ADR_tracks.txt"]
    assert (a / "ADR_detections.txt").read_bytes() == (b / "ADR_detections.txt").read_bytes()
    iq = formats.read_adc_pairs(GOLDEN / "golden_input_chirp.txt")
    with RadarCore(N_RANGE=256, N_DOPPLER=128, cfar="os1d") as core:
        out = core.process(synth.golden_chirp_frame(iq, 128, 256)[None])
    with TwsTracker() as trk:
        hist = [(trk.scan(out.dets), trk.active_tracks)]
    formats.write_tracks(tmp_path / "want_tracks.txt", hist)
    assert (a / "ADR_tracks.txt").read_bytes() == (tmp_path / "want_tracks.txt").read_bytes()
    want = plots_ref(out.dets, 256, 128, 1, 2)
    got = formats.read_plots(b / "ADR_plots.txt")
    assert len(got) == len(want) > 0
    np.testing.assert_array_equal(got[:, :3], np.stack([want["frame"], want["range"], want["doppler"]], 1))
    np.testing.assert_array_equal(got[:, 3], np.rint(want["mag"].astype(np.float64)))
    np.testing.assert_array_equal(got[:, 4], want["n_cells"])
    np.testing.assert_allclose(got[:, 5], want["range"] + want["d_range"], atol=1e-4 + 5e-4)   # 3 decimals
    np.testing.assert_allclose(got[:, 6], want["doppler"] + want["d_doppler"], atol=1e-4 + 5e-4)
