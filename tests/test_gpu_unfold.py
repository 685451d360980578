"""Velocity unfolding on the GPU (fmcw_unfold_* of libfmcw.so on gfx950 through the C-ABI), every case
against tests/unfold_ref.py (the specification in integers) run on the same list: record for record,
every field, mag and sum_mag bit for bit, and status word for status word.

Every output and status buffer is guarded: the report buffer is filled with a sentinel and has slots
beyond out_cap, the status words sit between sentinel words.
"""
import functools
import itertools

import numpy as np
import pytest

import reclist_cases as RC
import scenario_ref as S
import tws_dev_ref as TR
from fmcw import DET_DTYPE, PLOT_DTYPE, TRACK_DTYPE, VPLOT_DTYPE, DeviceBuffer, DeviceTwsTracker, PlotExtractor, VelocityUnfolder
from plots_ref import assert_plots_match, plots_ref
from gpu_support import SENTINEL, Chain, Hip, run_rec_list
from tile_edge import TILE_EDGE_SIZES
from unfold_ref import (FIGHTER_FACT, TILE_EDGE_CFG, Cfg, assert_vplots_equal, fighter_fact, n_dwells, random_list, scenario_cfg,
                        tile_edge_list, unfold_ref)

pytestmark = pytest.mark.gpu

NR, NC, SCANS = 64, 32, 9
UNITS = {2: (8, 9), 3: (8, 9, 10), 4: (7, 8, 9, 11), 5: (7, 8, 9, 11, 13), 8: (7, 8, 9, 11, 13, 15, 16, 17)}


def unfolder(cfg: Cfg, max_recs, max_frames=None):
    return VelocityUnfolder(cfg.n_range, cfg.n_doppler, cfg.prf_units, cfg.prf_phase, cfg.step, cfg.zero_bin, cfg.v_max,
                            cfg.out_unit, (cfg.tol_range, cfg.tol_doppler), cfg.m_of, cfg.n_streams,
                            max_recs=max(max_recs, 1), max_frames=max_frames)


def run(uf, recs, n_scans, out_cap=None, rec_cap=None, n_word=None, K=4):
    """One fmcw_unfold_enqueue on a host list: (status words, reports written, the sentinel-filled
    output buffer's bytes after them).  The status words sit between guard words, four on each side."""
    def enqueue(dr, stride, rec_cap, dn, do, out_cap, ds):
        uf.enqueue(dr, stride, rec_cap, dn, n_scans, do, out_cap, ds)
    out_cap = max(K * len(recs), 1) if out_cap is None else out_cap   # a record reports in at most K dwells
    return run_rec_list(enqueue, recs, VPLOT_DTYPE, 4, out_cap, rec_cap, n_word, guards=(4, 4))


def check(recs, n_scans, cfg, grids=(0,), max_recs=None, **kw):
    want, beyond, tied = unfold_ref(recs, n_scans, cfg)
    first = None
    with unfolder(cfg, len(recs) if max_recs is None else max_recs) as uf:
        for grid in grids:
            uf.set_grid_for_test(grid)
            st, got, rest = run(uf, recs, n_scans, K=max(cfg.n_prf, 4), **kw)
            assert list(st) == [len(want), 0, beyond, tied], (grid, st, len(want), beyond, tied)
            assert_vplots_equal(got, want)
            assert np.all(rest == SENTINEL), grid
            first = first or (got.tobytes(), rest.tobytes())
            assert (got.tobytes(), rest.tobytes()) == first, f"grid {grid}: other bytes than grid {grids[0]}"
    return got, want


CASES = sorted({(K, step, m_of) for K in (2, 3, 4) for step in (1, K) for m_of in (1, K - 1, K)})


@pytest.mark.parametrize("K,step,m_of", CASES)
def test_random_lists(gpu, K, step, m_of):
    """64 x 32, 9 scans, 200-300 records with a few movers written where their velocity folds to: both
    strides, 1 and 2 streams, zero_bin 0 and Nc / 2, tolerances 0 and 2, v_max 0 and 3 Nc p_min, and
    one frame beyond the last scan."""
    p = UNITS[K]
    reports = 0
    for k, (dtype, ns, zb, tol, vm) in enumerate(itertools.product((DET_DTYPE, PLOT_DTYPE), (1, 2), (0, NC // 2), (0, 2),
                                                                  (0, 3 * NC * min(p)))):
        cfg = Cfg(n_range=NR, n_doppler=NC, prf_units=p, prf_phase=k % K, step=step, zero_bin=zb, v_max=vm,
                  out_unit=min(p), tol_range=tol, tol_doppler=tol, m_of=m_of, n_streams=ns)
        recs = random_list(1000 * K + k, SCANS * ns + 1, NR, NC, 250 - 40 * ns, dtype, cfg=cfg)
        assert 200 <= len(recs) <= 300, len(recs)
        _, want = check(recs, SCANS, cfg)
        reports += len(want)
    assert reports > 0


@pytest.mark.parametrize("K,step,m_of", sorted({(K, step, m_of) for K in (5, 8) for step in (1, K) for m_of in (1, K - 1, K)}))
def test_random_lists_five_and_eight_prfs(gpu, K, step, m_of):
    """K = 5 and 8 (the second word of PRF units, positions 4..7 of hit_mask): 64 x 32, 2 K + 1 scans, 200-300
    records with movers, both strides, 1 and 2 streams; zero_bin, the tolerances and v_max take their two values
    in turn.  Some report has a hit at a position >= 4, and some has all K."""
    p = UNITS[K]
    high = full = 0
    for k, (dtype, ns) in enumerate(itertools.product((DET_DTYPE, PLOT_DTYPE), (1, 2))):
        j = k + step + m_of
        tol = (0, 2)[j % 2]
        cfg = Cfg(n_range=NR, n_doppler=NC, prf_units=p, prf_phase=j % K, step=step, zero_bin=(0, NC // 2)[j // 2 % 2],
                  v_max=(3 * NC * min(p), 0)[(j + k // 2) % 2 if k % 2 else 0], out_unit=min(p), tol_range=tol, tol_doppler=tol,
                  m_of=m_of, n_streams=ns)
        n_scans = 2 * K + 1
        recs = random_list(2000 * K + k, n_scans * ns + 1, NR, NC, 200, dtype, cfg=cfg, targets=3)
        assert 200 <= len(recs) <= 300, len(recs)
        _, want = check(recs, n_scans, cfg, grids=(0, 1) if k == 0 else (0,))
        high += int((want["hit_mask"] >> 4).astype(bool).sum())
        full += int((want["n_hits"] == K).sum())
    assert high > 0 and full > 0, (high, full)


def test_v_max_limit_65_hypotheses(gpu):
    """K = 3 at the admitted v_max limit 32 Nc p_min, 32 x 32 x 8 scans: 65 hypotheses per record."""
    cfg, recs = RC.unfold_v_max_limit_case()
    _, want = check(recs, 8, cfg, grids=(1, 0))
    assert len(want) > 0 and want["n_ties"].max() > 1 and np.abs(want["fold"]).max() >= 16


@pytest.mark.parametrize("dtype", [DET_DTYPE, PLOT_DTYPE], ids=["stride16", "stride32"])
def test_corner_list_at_the_limits(gpu, dtype):
    """n_range = n_doppler = 65536, records at the four corners and their neighbours across the Doppler wrap,
    PRF units 4096 / 4095 / 4093, tolerances of 4 and a v_max within 2^17 of 2^31 (reclist_cases.py; the list
    layer ran the same list on the CPU under sanitizers, test_reclist_replay.py).  max_recs is the list's length."""
    _, want = check(RC.unfold_corner_list(dtype), RC.UNFOLD_CORNER_SCANS, RC.UNFOLD_CORNER_CFG, grids=(1, 0))
    assert (want["n_hits"] == 3).sum() >= 4 and np.abs(want["v_fine"].astype(np.int64)).max() > 2 ** 31 - 2 ** 17


@functools.lru_cache(maxsize=None)
def long_list():
    """9 scans of 64 x 32 at about 333 records per frame: 3 tiles of records, frames and dwells across the
    tile boundaries."""
    cfg = Cfg(n_range=NR, n_doppler=NC, v_max=3 * NC * 8, step=3)
    recs = random_list(77, SCANS, NR, NC, 2700, PLOT_DTYPE, cfg=cfg, targets=40)
    assert 2 * 1024 < len(recs) <= 3 * 1024
    recs.setflags(write=False)
    return recs


@pytest.mark.parametrize("step", [3, 1])
def test_tiles_and_grid(gpu, step):
    """About 3000 records under one workgroup and under the built-in grid: with step 3 one workgroup walks
    three 1024-pair tiles, with step 1 (every record in up to three dwells) seven; the same bytes."""
    cfg = Cfg(n_range=NR, n_doppler=NC, v_max=3 * NC * 8, step=step)
    got, want = check(long_list(), SCANS, cfg, grids=(1, 0, 3))
    assert len(want) > 600 and (want["n_hits"] == 3).sum() > 10   # reports in every tile


def test_out_cap_shorter_than_count(gpu):
    cfg = Cfg(n_range=NR, n_doppler=NC, v_max=3 * NC * 8, step=1)
    recs = long_list()
    want, _, tied = unfold_ref(recs, SCANS, cfg)
    cap = len(want) // 3
    with unfolder(cfg, len(recs)) as uf:
        for grid in (0, 1):
            uf.set_grid_for_test(grid)
            st, got, rest = run(uf, recs, SCANS, out_cap=cap)
            assert list(st) == [len(want), 0, 0, tied]
            assert_vplots_equal(got, want[:cap])
            assert np.all(rest == SENTINEL)          # the slot after the prefix is untouched
        # unfold() reruns once with the reported count
        assert_vplots_equal(uf.unfold(recs, SCANS, out_cap=cap), want)
        assert list(uf.status) == [len(want), 0, 0, tied]
        st, got, rest = run(uf, recs, SCANS, out_cap=0)
        assert list(st) == [len(want), 0, 0, tied] and np.all(rest == SENTINEL)


def test_empty_list(gpu):
    with unfolder(Cfg(n_range=NR, n_doppler=NC, v_max=512), 64) as uf:
        st, got, rest = run(uf, np.zeros(0, DET_DTYPE), SCANS, out_cap=8)
        assert list(st) == [0, 0, 0, 0] and len(got) == 0 and np.all(rest == SENTINEL)
        # a count word above a zero rec_cap: nothing examined, everything reported as not examined
        st, got, rest = run(uf, np.zeros(0, DET_DTYPE), SCANS, out_cap=8, n_word=7)
        assert list(st) == [0, 7, 0, 0] and np.all(rest == SENTINEL)
        # records on the device, a zero count word
        recs = random_list(5, SCANS, NR, NC, 60, DET_DTYPE)
        st, got, rest = run(uf, recs, SCANS, out_cap=8, n_word=0)
        assert list(st) == [0, 0, 0, 0] and np.all(rest == SENTINEL)


def test_truncated_input(gpu):
    """n_recs_dev[0] above rec_cap, and above max_recs: the first n records are examined, word [1] counts
    the rest, and the reports equal the reference on the truncated list."""
    cfg = Cfg(n_range=NR, n_doppler=NC, v_max=3 * NC * 8, step=1)
    recs = long_list()
    n = len(recs)
    for rec_cap, max_recs in ((n - 700, n), (n, 1500)):
        cut = min(rec_cap, max_recs)
        want, beyond, tied = unfold_ref(recs[:cut], SCANS, cfg)
        with unfolder(cfg, max_recs) as uf:
            st, got, rest = run(uf, recs, SCANS, rec_cap=rec_cap, n_word=n + 5)
        assert list(st) == [len(want), n + 5 - cut, beyond, tied]
        assert_vplots_equal(got, want)
        assert np.all(rest == SENTINEL)


@pytest.mark.parametrize("n_scans", [0, 2, 3, 5, 8])
def test_frames_beyond_n_scans_and_too_few_scans(gpu, n_scans):
    """A 9-scan list of 2 streams unfolded as 0, 2, 3, 5 and 8 scans: the later frames are a suffix, counted in
    status word 2 and ignored; max_frames = n_scans * n_streams, so the index has no word for them.  With
    fewer than K = 3 scans there is no dwell: status only."""
    cfg = Cfg(n_range=NR, n_doppler=NC, v_max=3 * NC * 8, step=2, n_streams=2)
    recs = random_list(6, SCANS * 2, NR, NC, 280, DET_DTYPE, cfg=cfg)
    want, beyond, tied = unfold_ref(recs, n_scans, cfg)
    assert beyond > 0 and (len(want) > 0) == (n_scans >= 3)
    with unfolder(cfg, len(recs), max_frames=max(n_scans, 1) * 2) as uf:
        for grid in (0, 1):
            uf.set_grid_for_test(grid)
            st, got, rest = run(uf, recs, n_scans)
            assert list(st) == [len(want), 0, beyond, tied]
            assert_vplots_equal(got, want)
            assert np.all(rest == SENTINEL)


@pytest.mark.parametrize("n", TILE_EDGE_SIZES)
def test_index_at_its_tile_edge(gpu, n):
    """Lists of exactly 1023, 1024, 1025 and 2048 records (max_recs = n) that end in frame 3 of 6: the words
    of the empty frames 4 and 5 and start[n_frames] come from item i == n of the frame index, which at
    1024 and 2048 is alone in a tile of its own.  One workgroup and the built-in grid."""
    recs = tile_edge_list(n)
    got, want = check(recs, 6, TILE_EDGE_CFG, grids=(0, 1))
    assert len(want) > 0
    assert unfold_ref(recs, 6, TILE_EDGE_CFG)[1] == 0   # check() compared status word 2 with this


def test_n_scans_checked_before_the_launch(gpu):
    from fmcw import FmcwError
    with unfolder(Cfg(n_range=NR, n_doppler=NC, v_max=512, n_streams=2), 64, max_frames=6) as uf:
        with pytest.raises(FmcwError, match="n_scans"):
            uf.enqueue(0x1000, 16, 4, 0x1000, 4, 0x1000, 4, 0x1000)


def tracks_of(dt, dc, n_scans, cap):
    counts = dc.download(np.uint32, (n_scans, 2))
    tracks = dt.download(TRACK_DTYPE, (n_scans, cap))
    return [(tracks[m, :counts[m, 0]].copy(), int(counts[m, 1])) for m in range(n_scans)]


def test_graph_capture_plots_unfold_tracker(gpu):
    """fmcw_plots_enqueue -> fmcw_unfold_enqueue -> fmcw_tws_dev_enqueue (stride 32, the default gates, one
    tracker scan per dwell) captured into one graph on one stream.  A direct launch and a replay give the
    same plots and reports, each equal to its reference on the previous stage's output; the tracker's
    file lives on the device, so the replay after a reset equals the direct run and a second replay
    carries on from it, as the tracker's oracle does."""
    cfg = Cfg(n_range=NR, n_doppler=NC, v_max=3 * NC * 8, step=1)
    dets = random_list(8, SCANS, NR, NC, 280, DET_DTYPE, cfg=cfg)
    nd, cap, tcap = n_dwells(SCANS, 3, 1), 1024, 32
    hip = Hip()
    with PlotExtractor(NR, NC, win=(1, 1), max_dets=cap) as px, unfolder(cfg, cap) as uf, \
            DeviceTwsTracker(n_streams=1, max_scans=nd) as trk:
        dd, dn = DeviceBuffer(cap * 16), DeviceBuffer(16)
        dp, dps = DeviceBuffer(cap * 32), DeviceBuffer(8)
        dv, dvs = DeviceBuffer(3 * cap * 32), DeviceBuffer(16)
        dt, dc, dts = DeviceBuffer(nd * tcap * 28), DeviceBuffer(nd * 8), DeviceBuffer(8)
        dd.upload(dets)
        dn.upload(np.array([len(dets), 0, 0, 0], np.uint32))
        s = hip.stream()

        def chain():
            px.enqueue(dd, cap, dn, dp, cap, dps, stream=s.value)
            uf.enqueue(dp, 32, cap, dps, SCANS, dv, 3 * cap, dvs, stream=s.value)
            trk.enqueue(dv, 32, 3 * cap, dvs, nd, dt, tcap, dc, dts, stream=s.value)

        def result():
            hip.ok(hip.lib.hipStreamSynchronize(s))
            ps, vs = dps.download(np.uint32, (2,)), dvs.download(np.uint32, (4,))
            plots = dp.download(PLOT_DTYPE, (int(ps[0]),))
            return plots, vs, dv.download(VPLOT_DTYPE, (int(vs[0]),)), tracks_of(dt, dc, nd, tcap), dts.download(np.uint32, (2,))
        try:
            chain()
            plots, vs, vplots, tracks, ts = result()
            assert_plots_match(plots, plots_ref(dets, NR, NC, 1, 1))
            want, beyond, tied = unfold_ref(plots, SCANS, cfg)
            assert list(vs) == [len(want), 0, beyond, tied] and len(want) > nd
            assert_vplots_equal(vplots, want)
            assert np.all(np.diff(vplots["frame"].astype(np.int64)) >= 0) and int(vplots["frame"].max()) == nd - 1
            oracles = TR.make_oracles(1, False)
            ref1, _ = TR.run_ref(vplots, nd, 1, oracles)
            ref2, _ = TR.run_ref(vplots, nd, 1, oracles)       # the same scans again on the same track file

            def same(got, ref):
                return all(TR.tracks_equal(got[m][0], ref[m][0][0]) and got[m][1] == ref[m][0][1] for m in range(nd))
            assert list(ts) == [0, 0] and same(tracks, ref1) and max(len(t[0]) for t in tracks) > 0
            trk.reset(stream=s.value)
            with hip.graph(lambda s: chain(), s) as (exe, _):
                for ref in (ref1, ref2):
                    for b in (dp, dv):
                        b.upload(np.full(b.nbytes, SENTINEL, np.uint8))
                    hip.replay(exe, s)
                    plots_r, vs_r, vplots_r, tracks_r, ts_r = result()
                    assert plots_r.tobytes() == plots.tobytes() and list(vs_r) == list(vs)
                    assert vplots_r.tobytes() == vplots.tobytes()
                    assert list(ts_r) == [0, 0] and same(tracks_r, ref)
                assert not same(tracks_r, ref1)                      # the second replay did advance
        finally:
            hip.lib.hipStreamDestroy(s)
            for b in (dd, dn, dp, dps, dv, dvs, dt, dc, dts):
                b.free()


def test_scenario_chain(gpu):
    """CHAIN_SCENE through gpu_support.Chain (fmcw_enqueue behind the 2-pulse canceller ->
    fmcw_plots_enqueue) to the plot list; the unfolder on that list equals unfold_ref on it, and the
    fighter fact pinned on the CPU (unfold_ref.FIGHTER_FACT) holds on it."""
    sc, hip = S.CHAIN_SCENE, Hip()
    ch = Chain(hip, sc, sc.n_scans, 1, False)
    try:
        ch.cube.upload(np.ascontiguousarray(S.scene_cubes(sc)[0]))
        ch.clear()
        ch.enqueue()
        plots = ch.result()["plots"]
    finally:
        ch.close()
    cfg = scenario_cfg(sc)
    want, beyond, tied = unfold_ref(plots, sc.n_scans, cfg)
    with unfolder(cfg, len(plots)) as uf:
        got = uf.unfold(plots, sc.n_scans)
        assert list(uf.status) == [len(want), 0, beyond, tied]
    assert_vplots_equal(got, want)
    qualifying, holds, reports = fighter_fact(sc, plots, got)
    assert (qualifying, holds) == FIGHTER_FACT[sc.id]
    assert all(int(reports[j]["n_hits"]) == 3 for j in qualifying)
