"""The device tracker on the GPU (fmcw_tws_dev_* of libfmcw.so on gfx950 through the C-ABI).

Expected values come from tests/tws_dev_ref.py (one oracle/tws_oracle.TwsOracle per stream over the
list sliced into (scan, stream) groups); the host TwsTracker is a second check where a test says so.
Everything is integer arithmetic, so every comparison is equality: each fmcw_track field, n_out and
n_active of every (scan, stream), both status words, and the sentinel bytes of every track slot beyond
n_out.  No tolerance anywhere.

The frame index (k_frame_index, csrc/rec_tiles.hpp) works on tiles of 1024 items (kIdxTile): item i compares records
i - 1 and i, so a frame boundary "at records 1023 / 1024" is the first item of the second tile.
"""
import functools

import numpy as np
import pytest

import tws_oracle as T
import tws_dev_ref as R
from fmcw import DET_DTYPE, PLOT_DTYPE, DeviceBuffer, FmcwError, PlotExtractor, RadarCore, TwsTracker, synth
from gpu_support import GUARD, RTL, SENTINEL, Hip, assert_matches, sentinel_buffer, tracker

pytestmark = pytest.mark.gpu

TILE = 1024


def to_records(streams, dtype=DET_DTYPE, first_scan=0):
    """streams[s][k] = the (range, doppler, mag) list of scan k of stream s -> the ordered record list
    (frame = (first_scan + k) * n_streams + s)."""
    ns = len(streams)
    rows = [((first_scan + k) * ns + s, r, d, m) for k in range(len(streams[0])) for s in range(ns)
            for r, d, m in streams[s][k]]
    a = np.zeros(len(rows), dtype)
    if rows:
        f, r, d, m = zip(*rows)
        a["frame"], a["range"], a["doppler"], a["mag"] = f, r, d, m
    return a


def run_dev(trk, recs, n_scans, track_cap=None, rec_cap=None, n_word=None):
    """One fmcw_tws_dev_enqueue on a host list.  Returns (status words, counts [groups][2], the
    sentinel-filled track buffer's bytes [groups][track_cap x 28], the counts' two guard words)."""
    n, ns = len(recs), trk.cfg.n_streams
    cap = trk.cfg.tws.max_tracks if track_cap is None else track_cap
    groups = n_scans * ns
    dr = DeviceBuffer(max(recs.nbytes, 4))
    if n:
        dr.upload(recs)
    dn = DeviceBuffer(16)
    dn.upload(np.array([n if n_word is None else n_word, 0, 0, 0], np.uint32))
    dt = sentinel_buffer(max(groups, 1) * cap * 28)
    dc = sentinel_buffer((2 * groups + 2) * 4)
    ds = DeviceBuffer(8)
    ds.upload(np.array([0xDEAD, 0xBEEF], np.uint32))
    try:
        trk.enqueue(dr, recs.dtype.itemsize, n if rec_cap is None else rec_cap, dn, n_scans, dt, cap, dc, ds)
        st = ds.download(np.uint32, (2,))
        counts = dc.download(np.uint32, (2 * groups + 2,))
        raw = dt.download(np.uint8, (max(groups, 1), cap * 28))
    finally:
        for b in (dr, dn, dt, dc, ds):
            b.free()
    return st, counts[:2 * groups].reshape(groups, 2), raw, counts[2 * groups:]


def check(streams, rtl, grid=0, track_cap=None, dtype=DET_DTYPE, **params):
    """One call over all the scans of `streams` against fresh oracles; returns the device's results."""
    ns, n_scans = len(streams), len(streams[0])
    recs = to_records(streams, dtype)
    want, status = R.run_ref(recs, n_scans, ns, R.make_oracles(ns, rtl, **params))
    with tracker(ns, n_scans, rtl, **params) as trk:
        trk.set_grid_for_test(grid)
        got = run_dev(trk, recs, n_scans, track_cap=track_cap)
    assert_matches(got, want, status, ns, params.get("max_tracks", 32) if track_cap is None else track_cap)
    return got


def random_scans(seed, n_scans=40, max_extra=8, burst=False):
    """tests/test_tracker.py's generator: six moving targets seen with probability 0.85, up to
    max_extra - 1 false alarms, and with burst a scan of 70 more detections every seventh scan."""
    rng = np.random.default_rng(seed)
    tgt = [[rng.integers(20, 1000), rng.integers(5, 120), rng.integers(-6, 7), rng.integers(-2, 3)]
           for _ in range(6)]
    scans = []
    for s in range(n_scans):
        d = []
        for t in tgt:
            t[0] = int(np.clip(t[0] + t[2] + rng.integers(-1, 2), 0, 1023))
            t[1] = int(np.clip(t[1] + t[3] + rng.integers(-1, 2), 0, 127))
            if rng.random() < 0.85:
                d.append((t[0], t[1], int(rng.integers(1000, 200000))))
        for _ in range(int(rng.integers(0, max_extra))):
            d.append((int(rng.integers(0, 1024)), int(rng.integers(0, 128)), int(rng.integers(100, 5000))))
        if burst and s % 7 == 3:       # > 64 detections: the RTL's 6-bit counter wraps
            d += [(int(rng.integers(0, 1024)), int(rng.integers(0, 128)), 700) for _ in range(70)]
        rng.shuffle(d)
        scans.append(d)
    return scans


def sized(scans, sizes, seed=99):
    """A copy of `scans` whose scan k has exactly sizes[k] detections (cut, or filled with clutter)."""
    rng = np.random.default_rng(seed)
    out = [list(map(tuple, s)) for s in scans]
    for k, n in sizes.items():
        fill = [(int(rng.integers(0, 1024)), int(rng.integers(0, 128)), int(rng.integers(100, 5000)))
                for _ in range(max(0, n - len(out[k])))]
        out[k] = (out[k] + fill)[:n]
    return out


@functools.lru_cache(maxsize=None)
def burst_scans():
    """40 scans with the 70-detection bursts, and scans of exactly 0, 1, 63, 64 and 65 detections."""
    return sized(random_scans(9, burst=True), {5: 0, 6: 1, 12: 63, 13: 64, 14: 65})


@RTL
def test_tb_tws_tracker_scenario(gpu, rtl):
    """rtl/src/tb_tws_tracker.vhd's detections and generics (MAX_TRACKS 16, COAST_MAX 3), one call,
    one stream; the host tracker fed scan by scan is the second reference."""
    scans = T.tb_tws_scenario()
    _, counts, raw, _ = check([scans], rtl, max_tracks=16, coast_max=3)
    with TwsTracker(MAX_TRACKS=16, COAST_MAX=3, rtl_compat=rtl) as host:
        for k, dets in enumerate(scans):
            want = host.scan(np.array(dets, np.float64).reshape(-1, 3))
            assert (int(counts[k, 0]), int(counts[k, 1])) == (len(want), host.active_tracks)
            assert raw[k, :len(want) * 28].tobytes() == want.tobytes()
    assert int(counts[5, 1]) >= 3    # tb_tws_tracker.vhd: at least three tracks after scan 6


@RTL
@pytest.mark.parametrize("max_dets", [1, 8, 64])
def test_random_scans_max_dets(gpu, rtl, max_dets):
    """Truncation at max_dets; at 64 in RTL mode the 6-bit counter wraps on the 65- and 70+-detection
    scans (the 65th overwrites slot 0, INITIATE runs over count mod 64)."""
    check([burst_scans()], rtl, max_dets=max_dets)


@RTL
@pytest.mark.parametrize("max_tracks", [1, 16, 32, 64])
def test_random_scans_max_tracks(gpu, rtl, max_tracks):
    check([burst_scans()], rtl, max_tracks=max_tracks)


@RTL
def test_full_track_file(gpu, rtl):
    """More unclaimed detections than free slots: INITIATE fills the free slots in detection order
    and drops the rest; a track_cap below n_out stores the first track_cap tracks only."""
    scans = burst_scans()
    check([scans], rtl, max_tracks=8, init_hits=1, coast_max=2)
    got = check([scans], rtl, max_tracks=8, init_hits=1, coast_max=2, track_cap=3)
    if not rtl:     # (the RTL's association keeps at most one of these tracks firm)
        assert int(got[1][:, 0].max()) > 3


@RTL
def test_gate_and_gain_generics(gpu, rtl):
    check([random_scans(5, max_extra=3)], rtl, gate_r=3, gate_d=2, alpha_q8=200, beta_q8=30)
    check([random_scans(6)], rtl, gate_r=4096, gate_d=4096, alpha_q8=255, beta_q8=255, init_hits=0, coast_max=0)


@RTL
def test_equal_distance_ties(gpu, rtl):
    """Two detections equidistant from a track (the intended tracker takes the lower index, the RTL
    the last one), and one detection inside two tracks' gates (the lower slot claims it)."""
    a, b = (100, 40, 1000), (110, 60, 2000)
    scans = [[a, b], [a, b], [a, b],
             [(98, 40, 11), (102, 40, 12), b],            # +-2 range bins around track 0
             [(100, 39, 13), (100, 41, 14), (101, 40, 15), (99, 40, 16), b],   # four at distance 4
             [(105, 50, 17)], [(105, 50, 18)],            # inside both gates (10 x 5 bins), equidistant
             [a, b], [(104, 48, 19), (106, 52, 20)], [a, b]]
    check([scans], rtl)
    check([scans], rtl, max_tracks=2)


@RTL
def test_magnitude_edges_and_wide_positions(gpu, rtl):
    """The magnitude rounding's edges (0, negative, 0.5, the 17-bit wrap at 131071.5 and 131072, the
    clamp at 5e9), and ranges >= 1024 / Dopplers >= 128: the RTL's 10- and 7-bit fields wrap, the
    intended tracker keeps the wide values."""
    mags = [0.0, -1.0, 0.5, 131071.5, 131072.0, 5e9, 0.49, 3.0e9]
    scans = []
    for k in range(8):
        scans.append([(50 + 60 * i, 10 + 12 * i, mags[(i + k) % len(mags)]) for i in range(8)] +
                     [(1024 + 37 * k, 130 + k, 9.0), (65535, 65535, 70000.0), (4000 + 3 * k, 127, 131071.49),
                      (1023, 128 + 2 * k, 262143.0)])
    check([scans], rtl)


@RTL
def test_empty_frames(gpu, rtl):
    """Empty scans at the start, in the middle (runs of 1 and of 5) and at the end of the list: each
    is still a scan (the tracks coast and are dropped)."""
    base = random_scans(21, n_scans=24)
    scans = sized(base, {0: 0, 1: 0, 6: 0, 10: 0, 11: 0, 12: 0, 13: 0, 14: 0, 22: 0, 23: 0})
    check([scans], rtl, coast_max=3)
    check([scans, sized(base, {3: 0, 23: 0})], rtl, grid=1)


@RTL
def test_empty_list_and_status_words(gpu, rtl):
    """An entirely empty list (every scan coasts nothing: all counts 0); n_scans = 0 (only the status
    words are written); n_recs_dev[0] above rec_cap (status[0]); records at or beyond frame
    n_scans x n_streams (status[1]: counted, ignored)."""
    empty = np.zeros(0, DET_DTYPE)
    with tracker(2, 8, rtl) as trk:
        want, status = R.run_ref(empty, 6, 2, R.make_oracles(2, rtl))
        assert_matches(run_dev(trk, empty, 6), want, [0, 0], 2, 32)
    recs = to_records([random_scans(22, n_scans=10), random_scans(23, n_scans=10)])
    with tracker(2, 8, rtl) as trk:
        st, counts, raw, guard = run_dev(trk, recs, 0)
        assert list(st) == [0, len(recs)] and np.all(raw == SENTINEL) and list(guard) == [GUARD] * 2
        # n_scans = 0 left the track files at power-up: the next call is a fresh tracker's
        want, status = R.run_ref(recs, 8, 2, R.make_oracles(2, rtl))
        assert status[1] == int(np.sum(recs["frame"] >= 16)) > 0
        assert_matches(run_dev(trk, recs, 8), want, status, 2, 32)
    cap = len(recs) - 37
    with tracker(2, 10, rtl) as trk:
        want, status = R.run_ref(recs, 10, 2, R.make_oracles(2, rtl), rec_cap=cap)
        assert status == [37, 0]       # the helper knows the list's length; the count word claims 5 more
        with pytest.raises(AssertionError):
            R.run_ref(recs[::-1], 10, 2, R.make_oracles(2, rtl))      # the helper insists on the precondition
        st, counts, raw, guard = run_dev(trk, recs, 10, rec_cap=cap, n_word=len(recs) + 5)
    assert_matches((st, counts, raw, guard), want, [37 + 5, 0], 2, 32)


@RTL
def test_n_scans_above_max_scans_is_rejected(gpu, rtl):
    recs = to_records([random_scans(24, n_scans=3)])
    with tracker(1, 2, rtl) as trk:
        with pytest.raises(FmcwError, match="n_scans"):
            run_dev(trk, recs, 3)


@functools.lru_cache(maxsize=None)
def stream_scans(n_streams):
    """Random streams (one with bursts; an empty and a 65-detection scan each), except streams 0 and 2:
    one jittering target and nothing else, so that the stream's last active track associates in most
    scans and leaves its own distance in best_distance for the next scan."""
    streams = [sized(random_scans(30 + s, n_scans=12, burst=(s == 1)), {s: 0, 5 + s: 65}) for s in range(n_streams)]
    for s in (0, 2):
        rng = np.random.default_rng(70 + s)
        streams[s] = [[(300 * (s + 1) + int(rng.integers(-3, 4)), 40 + int(rng.integers(-2, 3)), 900)] for _ in range(12)]
    return streams


@RTL
@pytest.mark.parametrize("n_streams", [3, 5])
def test_streams(gpu, rtl, n_streams):
    """Interleaved frames of 3 and 5 independent track files: equal to one oracle per stream, and the
    same bytes under 1 and 2 workgroups (one wave runs several streams one after the other, its
    registers reloaded from the state block) as under the built-in grid.  In RTL mode each stream
    carries its own best_distance: the value the oracles carry out of a scan differs between the
    streams in several scans, so a shared one would show."""
    streams = stream_scans(n_streams)
    ref = check(streams, rtl)
    for grid in (1, 2):
        got = check(streams, rtl, grid=grid)
        for a, b in zip(got, ref):
            assert a.tobytes() == b.tobytes(), grid
    if rtl:
        carried = []
        for o, scans in zip(R.make_oracles(n_streams, True), streams):
            carried.append([(o.scan([(r, d, R.round_mag(m)) for r, d, m in dets]), o.best_distance)[1] for dets in scans])
        assert sum(len(set(at_scan)) > 1 for at_scan in zip(*carried)) >= 3


@RTL
def test_index_kernel_beyond_its_first_tile(gpu, rtl):
    """2,500 records over 40 scans with one workgroup (three tiles of 1024 items one after the other):
    frames 0..15 hold 64 records each, so frame 16 starts exactly at record 1024 (the boundary between
    records 1023 and 1024 is the second tile's first item); frames 16..23 hold 128 each, frames 24..30
    are empty and frame 31 starts exactly at record 2048: the 7-frame gap straddles the tile edge and
    its seven start words come from the third tile's first item.  Frames 31..39 share the other 452."""
    sizes = {k: 64 for k in range(16)}
    sizes.update({k: 128 for k in range(16, 24)})
    sizes.update({k: 0 for k in range(24, 31)})
    sizes.update({k: 50 for k in range(31, 40)})
    sizes[39] += 2
    scans = sized(random_scans(40), sizes)
    recs = to_records([scans])
    assert len(recs) == 2500
    f = recs["frame"]
    assert (f[TILE - 1], f[TILE], f[2 * TILE - 1], f[2 * TILE]) == (15, 16, 23, 31)
    ref = check([scans], rtl)
    got = check([scans], rtl, grid=1)
    for a, b in zip(got, ref):
        assert a.tobytes() == b.tobytes()


@RTL
def test_state_across_calls_and_reset(gpu, rtl):
    """16 scans in one call equal 8 + 8 in two (the track files and, in RTL mode, best_distance live
    on the device between calls); after reset the first 8 equal a fresh tracker's."""
    streams = [random_scans(50, n_scans=16), random_scans(51, n_scans=16, burst=True)]
    whole = check(streams, rtl)
    first = to_records([s[:8] for s in streams])
    second = to_records([s[8:] for s in streams])
    with tracker(2, 8, rtl) as trk:
        a = run_dev(trk, first, 8)
        b = run_dev(trk, second, 8)
        assert np.concatenate([a[1], b[1]]).tobytes() == whole[1].tobytes()
        assert np.concatenate([a[2], b[2]]).tobytes() == whole[2].tobytes()
        trk.reset()
        c = run_dev(trk, first, 8)
        assert c[1].tobytes() == a[1].tobytes() and c[2].tobytes() == a[2].tobytes()


def synthetic_dets(seed=60, nf=6, nr=64, nd=32):
    """A detection list with a few compact clusters per frame that drift from frame to frame."""
    rng = np.random.default_rng(seed)
    rows = set()
    for f in range(nf):
        for r0, d0, v in ((10, 5, 1), (30, 20, -1), (50, 12, 2)):
            for dr in (-1, 0, 1):
                for dd in (-1, 0, 1):
                    if rng.random() < 0.8 or (dr, dd) == (0, 0):
                        rows.add((f, r0 + v * f + dr, (d0 + dd) % nd, 100.0 - 30 * (abs(dr) + abs(dd)) + r0))
        rows.add((f, int(rng.integers(0, nr)), int(rng.integers(0, nd)), 7.0))
    rows = sorted(rows)
    a = np.zeros(len(rows), DET_DTYPE)
    for i, (f, r, d, m) in enumerate(rows):
        a[i] = (f, r, d, m, 1.0)
    return a


@RTL
def test_plot_records(gpu, rtl):
    """fmcw_plot records (stride 32): the plots of a synthetic detection list give the tracks the
    host tracker gives when fed the same plots frame by frame."""
    nf = 6
    with PlotExtractor(64, 32, win=(1, 1)) as px:
        plots = px.extract(synthetic_dets(nf=nf))
    assert plots.dtype == PLOT_DTYPE and 3 * nf <= len(plots) < 5 * nf
    with tracker(1, nf, rtl, init_hits=1) as trk:
        st, counts, raw, _ = run_dev(trk, plots, nf)
    assert list(st) == [0, 0] and int(counts[:, 0].max()) >= 3
    with TwsTracker(INIT_HITS=1, rtl_compat=rtl) as host:
        for f in range(nf):
            want = host.scan(plots[plots["frame"] == f])
            assert (int(counts[f, 0]), int(counts[f, 1])) == (len(want), host.active_tracks)
            assert raw[f, :len(want) * 28].tobytes() == want.tobytes()
            assert np.all(raw[f, len(want) * 28:] == SENTINEL)


@RTL
def test_end_to_end_on_the_device(gpu, rtl):
    """fmcw_enqueue (2-D CFAR, 4 frames of 64 chirps x 256 samples, two moving targets), then
    fmcw_plots_enqueue, then fmcw_tws_dev_enqueue on one stream with no host step between: the tracks
    equal the host tracker's on the downloaded plot list.  The same three calls captured into a graph
    and replayed twice equal two eager calls: the track files (and, in RTL mode, the best_distance the
    last active track of a call leaves in the state block) advance on every replay."""
    ns, nc, nf = 256, 64, 4
    cube = np.ascontiguousarray(synth.frames(nf, ns, nc, 1, "two_targets", seed=71))
    hip = Hip()
    cap, pcap, tcap = nf * ns * nc, 4096, 32
    with RadarCore(N_RANGE=ns, N_DOPPLER=nc, cfar="os2d", max_frames=nf) as core, \
            PlotExtractor(ns, nc, win=(1, 1), max_dets=cap) as px, tracker(1, nf, rtl, init_hits=1) as trk:
        dc = DeviceBuffer(cube.nbytes)
        dc.upload(cube)
        dd, dn = DeviceBuffer(cap * 16), DeviceBuffer(16)
        dp, dps = DeviceBuffer(pcap * 32), DeviceBuffer(16)
        dt, dcnt, dst = DeviceBuffer(nf * tcap * 28), DeviceBuffer(nf * 8), DeviceBuffer(8)
        s = hip.stream()

        def chain():
            core.enqueue(dc, nf, None, dd, cap, dn, stream=s.value)
            px.enqueue(dd, cap, dn, dp, pcap, dps, stream=s.value)
            trk.enqueue(dp, 32, pcap, dps, nf, dt, tcap, dcnt, dst, stream=s.value)

        def result():
            hip.ok(hip.lib.hipStreamSynchronize(s))
            return (dcnt.download(np.uint32, (nf, 2)).tobytes(), dt.download(np.uint8, (nf, tcap * 28)),
                    list(dst.download(np.uint32, (2,))))

        def clear():
            dt.upload(np.full(nf * tcap * 28, SENTINEL, np.uint8))
            hip.ok(hip.lib.hipStreamSynchronize(None))

        try:
            eager = []
            for _ in range(2):
                clear()
                chain()
                eager.append(result())
            n_plots = int(dps.download(np.uint32, (2,))[0])
            plots = dp.download(PLOT_DTYPE, (n_plots,))
            assert 0 < n_plots <= pcap and eager[0][2] == [0, 0]
            with TwsTracker(INIT_HITS=1, rtl_compat=rtl) as host:      # two passes over the same four frames
                for counts, raw, _ in eager:
                    counts = np.frombuffer(counts, np.uint32).reshape(nf, 2)
                    for f in range(nf):
                        want = host.scan(plots[plots["frame"] == f])
                        assert (int(counts[f, 0]), int(counts[f, 1])) == (len(want), host.active_tracks)
                        assert raw[f, :len(want) * 28].tobytes() == want.tobytes()
                        assert np.all(raw[f, len(want) * 28:] == SENTINEL)
            if not rtl:
                assert np.frombuffer(eager[0][0], np.uint32).reshape(nf, 2)[-1, 0] >= 1    # a firm track
                assert eager[0][0] != eager[1][0] or eager[0][1].tobytes() != eager[1][1].tobytes()
            trk.reset(stream=s.value)
            with hip.graph(lambda s: chain(), s) as (exe, _):
                for k in range(2):
                    clear()
                    hip.replay(exe, s)
                    got = result()
                    assert got[0] == eager[k][0] and got[1].tobytes() == eager[k][1].tobytes() and got[2] == [0, 0], k
        finally:
            hip.lib.hipStreamDestroy(s)
            for b in (dc, dd, dn, dp, dps, dt, dcnt, dst):
                b.free()
