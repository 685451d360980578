"""Beam merge on the GPU (fmcw_merge_* of libfmcw.so on gfx950 through the C-ABI), every case against
tests/merge_ref.py (the specification in NumPy, fp64 sums) run on the same list.

Tolerances (merge_ref.assert_mplots_match / tolerances): count, order, frame, range, doppler, beam,
n_merged and the bits of mag exact; with N the case's largest n_merged and u = 2^-24, sum_mag within
N u relative and each offset within 2 N u win bins (derived in merge_ref.tolerances).

Every output and status buffer is guarded: the plot buffer is filled with a sentinel and has slots
beyond out_cap, the status words sit between sentinel words.
"""
import functools

import numpy as np
import pytest

import fmcw_oracle as O
import reclist_cases as RC
import tws_dev_ref as TR
from fmcw import (DET_DTYPE, MPLOT_DTYPE, PLOT_DTYPE, BeamFormer, BeamMerger, BearingEstimator, DeviceBuffer,
                  DeviceTwsTracker, PlotExtractor, RadarCore, steering_weights, synth)
from beams_ref import assert_maps_match, beams_ref
from bearings_ref import assert_bearings_match, bearings_ref
from gpu_support import SENTINEL, Hip, run_rec_list
from merge_ref import HAND, assert_mplots_match, hand_records, merge_ref, random_list, tile_edge_list
from plots_ref import assert_plots_match, plots_ref
from tile_edge import TILE_EDGE_SIZES

pytestmark = pytest.mark.gpu


def as_plots(p):
    """plots_ref output (fp64 sums) re-packed as fmcw_plot records."""
    out = np.zeros(len(p), PLOT_DTYPE)
    for name in PLOT_DTYPE.names:
        out[name] = p[name]
    return out


def plots_per_map(dets, nr, nd, win=(1, 1)):
    return as_plots(plots_ref(dets, nr, nd, *win))


def run(mg, recs, n_maps, out_cap=None, rec_cap=None, n_word=None):
    """One fmcw_merge_enqueue on a host list: (status words, merged plots written, the sentinel-filled
    output buffer's bytes after them).  The status words sit between four guard words and one."""
    def enqueue(dr, stride, rec_cap, dn, do, out_cap, ds):
        mg.enqueue(dr, stride, rec_cap, dn, n_maps, do, out_cap, ds)
    out_cap = max(len(recs), 1) if out_cap is None else out_cap
    return run_rec_list(enqueue, recs, MPLOT_DTYPE, 3, out_cap, rec_cap, n_word, guards=(4, 1))


def check(recs, nr, nd, nb, win, wrap=False, n_maps=None, grids=(0,), **kw):
    if n_maps is None:
        n_maps = (int(recs["frame"].max()) // nb + 1) * nb if len(recs) else nb
    want, beyond = merge_ref(recs, nr, nd, nb, win, wrap, n_maps)
    first = None
    with BeamMerger(nr, nd, nb, win=win, beam_wrap=wrap, max_recs=max(len(recs), 1),
                    max_maps=max(n_maps, nb)) as mg:
        for grid in grids:
            mg.set_grid_for_test(grid)
            st, got, rest = run(mg, recs, n_maps, **kw)
            assert list(st) == [len(want), 0, beyond], (grid, st)
            assert_mplots_match(got, want, win)
            assert np.all(rest == SENTINEL), grid
            if first is None:
                first = (got.tobytes(), rest.tobytes())
            assert (got.tobytes(), rest.tobytes()) == first, f"grid {grid}: other bytes than grid {grids[0]}"
    return got, want


@pytest.mark.parametrize("dtype", [DET_DTYPE, PLOT_DTYPE], ids=["stride16", "stride32"])
@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_made_three_beams(gpu, name, dtype):
    rows, win, wrap, expect = HAND[name]
    got, _ = check(hand_records(rows, dtype), 8, 8, 3, win, bool(wrap))
    assert [tuple(int(p[k]) for k in ("frame", "beam", "range", "doppler", "n_merged")) for p in got] == expect


def test_widest_window_on_the_narrowest_map(gpu):
    """n_doppler 9 with windows (4, 4, 4) on 9 beams, wrapped: every row is the whole circular Doppler
    axis and every map of the scan is a neighbour (up to 9 * 9 * 9 = 729 records)."""
    recs = random_list(31, 18, 12, 9, 0.9)
    recs["mag"][np.flatnonzero((recs["frame"] == 4) & (recs["range"] == 6))[0]] = 9.0   # a peak with a whole neighbourhood
    got, want = check(recs, 12, 9, 9, (4, 4, 4), True)
    assert want["n_merged"].max() > 600
    check(recs, 12, 9, 9, (4, 4, 4), False)


@pytest.mark.parametrize("nb,win,wrap", [(1, (1, 1, 1), 0), (1, (4, 1, 1), 0), (2, (1, 1, 1), 0), (2, (4, 1, 1), 0),
                                         (3, (1, 1, 1), 1), (3, (4, 0, 1), 0), (9, (4, 1, 0), 1), (64, (1, 1, 1), 1),
                                         (64, (4, 1, 1), 0)])
def test_beam_counts(gpu, nb, win, wrap):
    """1, 2, 3 and 64 beams; win_beam at or above the number of beams (clamped: every beam of the scan
    is a neighbour); the wrap at n_beams = 2 win_beam + 1 (3 with 1, 9 with 4)."""
    scans = 2 if nb < 64 else 1
    recs = random_list(32 + nb, scans * nb, 16, 12, 0.4 if nb < 64 else 0.1)
    check(recs, 16, 12, nb, win, bool(wrap))


@pytest.mark.parametrize("density", [0.05, 0.5, 1.0])
@pytest.mark.parametrize("stride", [16, 32])
def test_random_lists_over_all_window_triples(gpu, density, stride):
    """2 scans x 5 beams x 24 x 16, magnitudes from {1..5} so that ties are everywhere, every window
    triple from {0, 1, 4}, clamped and wrapped (where 5 beams allow it).  Stride 32: plots_ref's
    per-map output re-packed as fmcw_plot."""
    nb, nr, nd = 5, 24, 16
    recs = random_list(33, 2 * nb, nr, nd, density)
    if stride == 32:
        recs = plots_per_map(recs, nr, nd, (0, 1))
    with_ties = 0
    for wb in (0, 1, 4):
        for wr in (0, 1, 4):
            for wd in (0, 1, 4):
                for wrap in (False, True):
                    if wrap and nb < 2 * wb + 1:
                        continue
                    got, want = check(recs, nr, nd, nb, (wb, wr, wd), wrap)
                    with_ties += int(len(want) > 0)
    assert with_ties


@functools.lru_cache(maxsize=None)
def straddling_list():
    """2 scans x 3 beams x 64 x 32 at density 0.9: about 1840 records per map, so a map's segment spans
    tile boundaries (1024 records) and a record's neighbours in the next beam lie a whole map -- more
    than the 512-record halo, and mostly another tile -- away.  About 11 tiles."""
    recs = random_list(34, 6, 64, 32, 0.9)
    per_map = np.bincount(recs["frame"], minlength=6)
    assert per_map.min() > 1024 + 512 and len(recs) > 10 * 1024
    recs.setflags(write=False)
    return recs


@pytest.mark.parametrize("win,wrap", [((1, 1, 1), False), ((1, 4, 4), True), ((4, 1, 1), False)])
def test_maps_straddle_tiles_and_halo_under_capped_grids(gpu, win, wrap):
    """The straddling list under the built-in grid and under 1 and 3 workgroups
    (fmcw_merge_set_grid_for_test: every tile after another on the same staging arrays; 3 does not
    divide the tile count): the reference's merged plots, and the same bytes each time."""
    check(straddling_list(), 64, 32, 3, win, wrap, grids=(0, 1, 3))


def test_scan_beyond_its_first_round(gpu):
    """More than 1024 tiles: k_merge_scan takes a second round, and tile 1024's offset is the first
    round's total.  16 maps (2 scans x 8 beams) of 1024 x 128 cells at density 0.55 cut to 1024 * 1024 +
    1 records; small integer magnitudes, so the fp32 sums are exact.  The built-in grid and 3
    workgroups."""
    nb, nr, nd, n = 8, 1024, 128, 1024 * 1024 + 1
    recs = random_list(35, 16, nr, nd, 0.55)[:n].copy()
    assert len(recs) == n
    recs["mag"][-1] = 9.0
    got, want = check(recs, nr, nd, nb, (1, 1, 0), True, n_maps=16, grids=(0, 3), out_cap=n // 2)
    key = lambda a, f: (f.astype(np.int64) * nr + a["range"]) * nd + a["doppler"]   # noqa: E731
    per_tile = np.bincount(np.searchsorted(key(recs, recs["frame"]), key(want, want["frame"] * nb + want["beam"])) // 1024,
                           minlength=1025)
    assert len(per_tile) == 1025 and per_tile.min() >= 1 and len(set(per_tile.tolist())) > 1
    for name in ("sum_mag", "d_beam", "d_range", "d_doppler"):
        np.testing.assert_array_equal(got[name], want[name].astype(np.float32), err_msg=name)


def test_empty_list(gpu):
    with BeamMerger(64, 32, 4) as mg:
        st, got, rest = run(mg, np.zeros(0, DET_DTYPE), 8, out_cap=8)
        assert list(st) == [0, 0, 0] and len(got) == 0 and np.all(rest == SENTINEL)
        # a count word above a zero rec_cap: nothing examined, everything reported as not examined
        st, got, rest = run(mg, np.zeros(0, DET_DTYPE), 8, out_cap=8, n_word=7)
        assert list(st) == [0, 7, 0] and np.all(rest == SENTINEL)


def test_out_cap_shorter_than_count(gpu):
    recs = random_list(36, 6, 64, 32, 0.3)
    want, _ = merge_ref(recs, 64, 32, 3, (1, 1, 1))
    cap = len(want) // 3
    assert len(recs) > 2048 and cap > 0
    with BeamMerger(64, 32, 3, max_recs=len(recs)) as mg:
        first = None
        for grid in (0, 1, 3):
            mg.set_grid_for_test(grid)
            st, got, rest = run(mg, recs, 6, out_cap=cap)
            assert list(st) == [len(want), 0, 0]
            assert_mplots_match(got, want[:cap], (1, 1, 1))
            assert np.all(rest == SENTINEL)
            first = first or got.tobytes()
            assert got.tobytes() == first
        # merge() reruns once with the reported count
        assert_mplots_match(mg.merge(recs, 6, out_cap=cap), want, (1, 1, 1))
        st, got, rest = run(mg, recs, 6, out_cap=0)
        assert list(st) == [len(want), 0, 0] and np.all(rest == SENTINEL)


def test_truncated_input(gpu):
    """n_recs_dev[0] above rec_cap, and above max_recs: the first n records are examined, word [1]
    counts the rest, and the merged plots equal the reference on the truncated list."""
    recs = random_list(37, 6, 64, 32, 0.3)
    n = len(recs)
    with BeamMerger(64, 32, 3, max_recs=n) as mg:                 # rec_cap binds
        cap = n - 700
        st, got, rest = run(mg, recs, 6, rec_cap=cap, n_word=n + 5)
    want, _ = merge_ref(recs[:cap], 64, 32, 3, (1, 1, 1), n_maps=6)
    assert list(st) == [len(want), n + 5 - cap, 0]
    assert_mplots_match(got, want, (1, 1, 1))
    assert np.all(rest == SENTINEL)
    mr = 1500
    with BeamMerger(64, 32, 3, max_recs=mr) as mg:                # max_recs binds
        st, got, rest = run(mg, recs, 6, rec_cap=n, n_word=n)
    want, _ = merge_ref(recs[:mr], 64, 32, 3, (1, 1, 1), n_maps=6)
    assert list(st) == [len(want), n - mr, 0]
    assert_mplots_match(got, want, (1, 1, 1))
    assert np.all(rest == SENTINEL)


@pytest.mark.parametrize("n_maps", [0, 3, 6])
def test_records_beyond_n_maps(gpu, n_maps):
    """A list of 3 scans x 3 beams merged with n_maps 0, 3 and 6: the records of the later scans are
    counted in status word 2 and ignored; max_maps = n_maps, so the map index has no word for them."""
    recs = random_list(38, 9, 32, 16, 0.4)
    got, want = check(recs, 32, 16, 3, (1, 1, 1), True, n_maps=n_maps, grids=(0, 1))
    assert len(want) > 0 or n_maps == 0


def test_empty_maps_in_the_middle_of_a_scan(gpu):
    """Beams 1 and 3 of scan 0 and the whole of scan 1 hold no record: their map-index words come from
    the neighbouring records' store loops, and a neighbour search in them finds nothing."""
    recs = random_list(39, 15, 32, 16, 0.4)
    recs = recs[~np.isin(recs["frame"], [1, 3, 5, 6, 7, 8, 9])]
    for wrap in (False, True):
        check(recs, 32, 16, 5, (2, 1, 1), wrap, n_maps=15)
    check(recs[recs["frame"] >= 4], 32, 16, 5, (1, 1, 1), True, n_maps=15)    # a leading gap of four maps


@pytest.mark.parametrize("n", TILE_EDGE_SIZES)
def test_index_at_its_tile_edge(gpu, n):
    """Lists of exactly 1023, 1024, 1025 and 2048 records (max_recs = n) that end in map 3 of 6: the words
    of the empty maps 4 and 5 and start[n_maps] come from item i == n of the frame index, which at 1024
    and 2048 is alone in a tile of its own.  The built-in grid and one workgroup."""
    recs = tile_edge_list(n)
    want, beyond = merge_ref(recs, 32, 32, 3, (1, 1, 1), False, 6)
    assert beyond == 0 and len(want) > 0
    with BeamMerger(32, 32, 3, win=(1, 1, 1), max_recs=n, max_maps=6) as mg:
        for grid in (0, 1):
            mg.set_grid_for_test(grid)
            st, got, rest = run(mg, recs, 6)
            assert list(st) == [len(want), 0, 0], (grid, st)
            assert_mplots_match(got, want, (1, 1, 1))
            assert np.all(rest == SENTINEL), grid


@pytest.mark.parametrize("wrap", [False, True])
@pytest.mark.parametrize("dtype", [DET_DTYPE, PLOT_DTYPE], ids=["stride16", "stride32"])
def test_corner_list_at_the_limits(gpu, dtype, wrap):
    """n_range = n_doppler = 65536, records at the four corners and their neighbours across the Doppler wrap in
    2 scans x 9 beams (and one map beyond them), windows (4, 4, 4) (reclist_cases.py; the list layer ran the same
    lists on the CPU under sanitizers, test_reclist_replay.py).  max_recs is the list's length; one workgroup
    and the built-in grid."""
    m = RC.MERGE_CORNER
    recs = RC.corner_list(m["n_maps"] + 1, dtype, seed=dtype.itemsize)
    got, want = check(recs, RC.LIMIT, RC.LIMIT, m["n_beams"], m["win"], wrap, n_maps=m["n_maps"], grids=(1, 0))
    assert len(want) > 0 and want["n_merged"].max() > 8


def test_n_maps_checked_before_the_launch(gpu):
    from fmcw import FmcwError
    with BeamMerger(32, 16, 3, max_maps=6) as mg:
        for n_maps, text in ((9, "max_maps"), (4, "n_beams")):
            with pytest.raises(FmcwError, match=text):
                mg.enqueue(0x1000, 16, 4, 0x1000, n_maps, 0x1000, 4, 0x1000)


def test_graph_capture_cfar_plots_merge(gpu):
    """fmcw_cfar (1-D OS-CFAR over 2 scans x 4 beam maps of 64 x 32), fmcw_plots_enqueue and
    fmcw_merge_enqueue captured once on one stream, replayed on a second set of maps and on the first
    again: every stage equals its reference on the previous stage's output, each time."""
    nr, nd, nb, scans = 64, 32, 4, 2
    n_maps = nb * scans
    rng = np.random.default_rng(40)

    def maps_of(seed):
        m = np.random.default_rng(seed).rayleigh(1.0, (n_maps, nr, nd)).astype(np.float32)
        for k in range(3):                                        # targets seen in neighbouring beams
            s, b, r, d = rng.integers(0, scans), rng.integers(0, nb - 1), rng.integers(8, nr - 8), rng.integers(0, nd)
            m[s * nb + b, r, d] += 40.0 + k
            m[s * nb + b + 1, r, d] += 30.0
        return m
    inputs = [maps_of(41), maps_of(42)]
    hip = Hip()
    cap = n_maps * nr * nd
    with RadarCore(N_RANGE=nr, N_DOPPLER=nd, cfar="os1d", max_frames=n_maps) as core, \
            PlotExtractor(nr, nd, win=(1, 1), max_dets=cap) as px, \
            BeamMerger(nr, nd, nb, win=(1, 1, 1), max_recs=cap, max_maps=n_maps) as mg:
        dm = DeviceBuffer(inputs[0].nbytes)
        dd, dn = DeviceBuffer(cap * 16), DeviceBuffer(16)
        dp, dps = DeviceBuffer(cap * 32), DeviceBuffer(8)
        do, dst = DeviceBuffer(cap * 32), DeviceBuffer(12)

        def chain(s):
            core.cfar(dm, n_maps, dd, cap, dn, stream=s.value)
            px.enqueue(dd, cap, dn, dp, cap, dps, stream=s.value)
            mg.enqueue(dp, 32, cap, dps, n_maps, do, cap, dst, stream=s.value)
        try:
            with hip.graph(chain) as (exe, s):
                seen = []
                for k in (0, 1, 0):
                    dm.upload(inputs[k])
                    hip.replay(exe, s)
                    n = int(dn.download(np.uint32, (4,))[0])
                    dets = dd.download(DET_DTYPE, (n,))
                    want_p = plots_ref(dets, nr, nd, 1, 1)
                    ps = dps.download(np.uint32, (2,))
                    assert n > 0 and list(ps) == [len(want_p), 0], (k, n, ps)
                    plots = dp.download(PLOT_DTYPE, (len(want_p),))
                    assert_plots_match(plots, want_p)
                    want_m, _ = merge_ref(plots, nr, nd, nb, (1, 1, 1), n_maps=n_maps)
                    st = dst.download(np.uint32, (3,))
                    assert list(st) == [len(want_m), 0, 0] and 0 < len(want_m) < len(plots), (k, st)
                    got = do.download(MPLOT_DTYPE, (len(want_m),))
                    assert_mplots_match(got, want_m, (1, 1, 1))
                    seen.append(got.tobytes())
                assert seen[0] == seen[2] and seen[0] != seen[1]   # the replays saw their own maps
        finally:
            for b in (dm, dd, dn, dp, dps, do, dst):
                b.free()


# ---- end to end: range FFT -> beams -> CFAR -> plots -> merge -> tracker / bearings ----
E_NR, E_NC, E_NRX, E_NB, E_NF = 256, 64, 4, 8, 4
E_NUS = (np.arange(E_NB) - E_NB // 2) / E_NB       # 8 DFT beams over 4 channels: beams overlap 2 : 1
E_PHASES = [0.17, -0.25]                          # target 1 between beams 5 and 6 (5.36), target 2 on beam 2
E_CELLS = [(25, 5), (125, E_NC - 10)]             # two_targets at 256 x 64
E_WIN = (3, 4, 4)                                 # +-3 beams: the 4-element pattern's first sidelobes


def firm_near(tracks, r, d, nd, gate_r=2, gate_d=2):
    n = 0
    for t in tracks:
        dr = abs(int(t["range_q2"]) / 4 - r)
        dv = abs(int(t["doppler_q2"]) / 4 - d)
        n += int(int(t["status"]) == 2 and dr <= gate_r and min(dv, nd - dv) <= gate_d)
    return n


def test_end_to_end_chain(gpu):
    """256 x 64, 4 rx, 8 DFT beams, 4 scans of two_targets (the first target between two beams):
    fmcw_range_ct -> BeamFormer -> fmcw_cfar -> PlotExtractor -> BeamMerger -> DeviceTwsTracker(1 stream),
    each stage against its reference on the previous stage's GPU output.  One firm track per target
    after the merge; without it (the references, one track file per beam) the first target is firm in
    more than one beam.  BearingEstimator on the merged plots reads spectrum frame f."""
    n_maps = E_NF * E_NB
    cube = np.ascontiguousarray(synth.frames(E_NF, E_NR, E_NC, E_NRX, "two_targets", seed=90, rx_phase=E_PHASES))
    w = steering_weights(E_NRX, E_NUS)
    cap = n_maps * E_NR * E_NC
    with RadarCore(N_RANGE=E_NR, N_DOPPLER=E_NC, N_RX=E_NRX, cfar="none", max_frames=E_NF) as rc, \
            BeamFormer(E_NR, E_NC, E_NRX, w) as bf, \
            RadarCore(N_RANGE=E_NR, N_DOPPLER=E_NC, N_RX=1, cfar="os1d", max_frames=n_maps) as core:
        dc = DeviceBuffer(cube.nbytes)
        dc.upload(cube)
        dspec = DeviceBuffer(E_NF * bf.spec_frame_bytes())
        dm = DeviceBuffer(E_NF * bf.maps_frame_bytes())
        dd, dn = DeviceBuffer(cap * 16), DeviceBuffer(16)
        try:
            rc.range_ct(dc, dspec, E_NF)
            bf.enqueue(dspec, E_NF, dm)
            core.cfar(dm, n_maps, dd, cap, dn)
            st = dn.download(np.uint32, (4,))
            spec = dspec.download(np.complex64, (E_NF, E_NRX, E_NR, E_NC))
            maps = dm.download(np.float32, (n_maps, E_NR, E_NC))
            dets = dd.download(DET_DTYPE, (int(st[0]),))
        finally:
            for b in (dc, dspec, dm, dd, dn):
                b.free()
    assert_maps_match(maps.reshape(E_NF, E_NB, E_NR, E_NC), *beams_ref(spec, w), label="end to end")
    want = []
    for m in range(n_maps):
        det, thr = O.cfar_os1d(maps[m], O.Cfar1D())
        want.append(O.detections(det, maps[m], thr, frame=m))
    np.testing.assert_array_equal(dets, np.concatenate(want))
    with PlotExtractor(E_NR, E_NC, win=E_WIN[1:], max_dets=len(dets)) as px:
        plots = px.extract(dets)
    assert_plots_match(plots, plots_ref(dets, E_NR, E_NC, *E_WIN[1:]))
    with BeamMerger(E_NR, E_NC, E_NB, win=E_WIN, beam_wrap=True, max_recs=len(plots), max_maps=n_maps) as mg:
        merged = mg.merge(plots, n_maps)
        pos = mg.beam_position(merged)
        u = mg.interp(merged, E_NUS, period=1.0)
    want_m, _ = merge_ref(plots, E_NR, E_NC, E_NB, E_WIN, True, n_maps)
    assert_mplots_match(merged, want_m, E_WIN)
    assert np.all(np.diff(merged["frame"].astype(np.int64)) >= 0) and merged["frame"].max() == E_NF - 1
    for (r, d), nu in zip(E_CELLS, E_PHASES):
        at = (merged["range"] == r) & (merged["doppler"] == d)
        assert at.sum() == E_NF, (r, d, merged[at])           # one merged plot per scan
        true = (nu * E_NB + E_NB // 2) % E_NB
        assert np.all(np.abs((pos[at] - true + E_NB / 2) % E_NB - E_NB / 2) <= 0.5), (pos[at], true)
        assert np.all(np.abs((u[at] - nu + 0.5) % 1.0 - 0.5) <= 0.5 / E_NB)
    # the tracker: one stream over the merged plots, against its oracle, one firm track per target
    with DeviceTwsTracker(n_streams=1, max_scans=E_NF) as trk:
        out = trk.run(merged.view(PLOT_DTYPE), E_NF)
        assert list(trk.status) == [0, 0]
    ref_out, _ = TR.run_ref(merged, E_NF, 1, TR.make_oracles(1, False))
    for scan in range(E_NF):
        assert TR.tracks_equal(out[scan][0][0], ref_out[scan][0][0]) and out[scan][0][1] == ref_out[scan][0][1]
    last = out[E_NF - 1][0][0]
    for r, d in E_CELLS:
        assert firm_near(last, r, d, E_NC) == 1, (r, d, last)
    # for contrast, the references alone: one track file per beam on the per-beam plots
    per_beam, _ = TR.run_ref(plots, E_NF, E_NB, TR.make_oracles(E_NB, False))
    r, d = E_CELLS[0]
    streams = 0
    for b in range(E_NB):
        for t in per_beam[E_NF - 1][b][0]:
            dv = abs(t["doppler_q2"] / 4 - d)
            if t["status"] == 2 and abs(t["range_q2"] / 4 - r) <= 2 and min(dv, E_NC - dv) <= 2:
                streams += 1
                break
    assert streams > 1, streams
    # bearings: the merged plots' frame is the scan, which is the spectrum frame
    with BearingEstimator(E_NR, E_NC, E_NRX, max_records=len(merged)) as be:
        got_b, snaps = be.estimate(spec, merged.view(PLOT_DTYPE))
    assert_bearings_match(got_b, snaps, *bearings_ref(spec, merged), label="merged plots")
    for (r, d), nu in zip(E_CELLS, E_PHASES):
        at = (got_b["range"] == r) & (got_b["doppler"] == d)
        assert np.all(np.abs(got_b["nu"][at] - nu) < 0.01), (got_b[at], nu)
