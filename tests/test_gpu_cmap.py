"""The clutter map on the GPU (fmcw_cmap_* of libfmcw.so on gfx950 through the C-ABI).  Lists, status
words, planes and ages are compared bit for bit with tests/cmap_ref.py (the header's specification in NumPy
float32).  Every run writes into sentinel-filled buffers and checks the records after the list.

Shapes are the smallest at which each mechanism can go wrong.  A tile is 8192 / n_doppler range rows (or
the whole plane): 64 x 32 is one tile; n_range 64 with n_doppler 32 .. 1024 gives 1 .. 8 tiles of 64 .. 8
rows, the halo rows of a neighbour tile, the clipped halo at rows 0 and 63 and the Doppler wrap; 8192 x 32
gives 32 tiles of 256 rows; 256 x 64 and 256 x 1024 with 2 streams give 4 and 64 (stream, tile) units for
the persistent loop.
"""
import numpy as np
import pytest

import cmap_ref as R
from fmcw import DET_DTYPE, BeamFormer, ClutterMap, DeviceBuffer, PlotExtractor, RadarCore, steering_weights, synth
from fmcw import _lib as L
from gpu_support import SENTINEL, Hip, rayleigh, run_map_detector

pytestmark = pytest.mark.gpu

CANARY = 8          # sentinel records kept after the list
AGE_MAX = R.AGE_MAX


def run(cm, maps, det_cap=None, null_dets=False):
    """One fmcw_cmap_enqueue on host maps: (the records written, the four status words), after
    checking that every record from min(found, det_cap) on kept the sentinel."""
    return run_map_detector(cm, maps, det_cap, null_dets, canary=CANARY)


def same_state(cm, planes, ages):
    gp, ga = cm.get_state()
    assert ga.tolist() == np.asarray(ages).tolist()
    assert gp.tobytes() == np.asarray(planes, np.float32).tobytes()


def check(maps, label="", max_frames=None, **kw):
    """A fresh map, one call: list, status words, planes and ages against the reference."""
    maps = np.asarray(maps, np.float32)
    nf, nr, nd = maps.shape
    want, planes, ages = R.detect(maps, **kw)
    with ClutterMap(nr, nd, max_frames=max_frames or nf, **kw) as cm:
        got, st = run(cm, maps)
        print(f"\n{label} {nr}x{nd}x{nf} {kw}: {len(want)} detections")
        assert st.tolist() == [len(want), 0, 0, 0]
        assert got.tobytes() == want.tobytes()
        same_state(cm, planes, ages)
    return want


def cells_of(dets, frame=None):
    d = dets if frame is None else dets[dets["frame"] == frame]
    return set(zip(d["range"].tolist(), d["doppler"].tolist()))


def test_basic_list_and_state(gpu):
    """64 x 32, 12 scans, warmup 3: alpha 2.5 detects a few cells; alpha 1 about a fifth of them with the
    default spread (the largest of 9 averages) and roughly half with spread 0/0 (the cell's own average)."""
    maps = rayleigh(12, 64, 32, 11)
    few = check(maps, "few", alpha=2.5, warmup=3)
    assert 0 < len(few) < 0.02 * 9 * 64 * 32 and few["frame"].min() >= 3
    fifth = check(maps, "fifth", alpha=1.0, warmup=3)
    assert 0.1 < len(fifth) / (9 * 64 * 32) < 0.3 and set(fifth["frame"].tolist()) == set(range(3, 12))
    half = check(maps, "half", alpha=1.0, warmup=3, spread=(0, 0))
    assert 0.3 < len(half) / (9 * 64 * 32) < 0.7 and set(half["frame"].tolist()) == set(range(3, 12))


def test_calls_split(gpu):
    """The same 12 scans as one call and as calls of 1, 2, 4 and 5 scans: equal lists once the frame
    offsets are added, equal state."""
    maps = rayleigh(12, 64, 32, 12)
    kw = dict(alpha=1.2, warmup=3, clip=2.0)
    want, planes, ages = R.detect(maps, **kw)
    with ClutterMap(64, 32, max_frames=12, **kw) as one, ClutterMap(64, 32, max_frames=5, **kw) as split:
        whole, st = run(one, maps)
        assert st[0] == len(want) > 0 and whole.tobytes() == want.tobytes()
        parts, off = [], 0
        for n in (1, 2, 4, 5):
            d, st = run(split, maps[off:off + n])
            assert st[0] == len(d)
            d["frame"] += off
            parts.append(d)
            off += n
        assert np.concatenate(parts).tobytes() == whole.tobytes()
        same_state(one, planes, ages)
        same_state(split, planes, ages)


@pytest.mark.parametrize("nd", [32, 64, 128, 256, 512, 1024])
def test_every_doppler_size(gpu, nd):
    """n_range 64, warmup 3, 5 scans.  Strong cells in the last scan at rows 0, 1, 62, 63 and Doppler 0,
    mid, n_doppler - 1 are detected.  Masking: cells held at 100 through every scan raise the threshold of
    their neighbourhood, so a target of 30 in the adjacent cell across the Doppler wrap and in the adjacent
    row is missed with spread 1/1 and found with spread 0/0; range does not wrap, so the target at row 0
    under a strong cell at row 63 is found with either."""
    nr, nf = 64, 5
    maps = rayleigh(nf, nr, nd, 100 + nd).copy()
    strong = [(r, d) for r in (0, 1, 62, 63) for d in (0, nd // 2 + 3, nd - 1)]
    for r, d in strong:
        maps[nf - 1, r, d] = 40.0
    held = [(30, 0), (40, nd - 1), (63, 9)]
    for r, d in held:
        maps[:, r, d] = 100.0
    masked = [(30, nd - 1), (31, 0), (29, 0), (40, 0), (39, nd - 1)]     # across the wrap and in the adjacent rows
    free = [(0, 9)]                                                      # row 63's neighbour only if range wrapped
    for r, d in masked + free:
        maps[nf - 1, r, d] = 30.0
    near = check(maps, "spread 1/1", alpha=4.0, warmup=3)
    last = cells_of(near, nf - 1)
    assert set(strong) | set(free) <= last and not (set(masked) & last)
    alone = check(maps, "spread 0/0", alpha=4.0, warmup=3, spread=(0, 0))
    assert set(strong) | set(free) | set(masked) <= cells_of(alone, nf - 1)
    check(maps, "dense", alpha=1.0, warmup=3)                            # about half the cells: their thresholds, bit for bit


@pytest.mark.parametrize("spread", [(0, 0), (4, 0), (0, 4), (4, 4)])
def test_spread_matrix(gpu, spread):
    maps = rayleigh(6, 64, 32, 21)
    assert len(check(maps, "plain", alpha=1.0, warmup=2, spread=spread)) > 0
    assert len(check(maps, "clip, floor", alpha=1.0, warmup=2, spread=spread, clip=2.0, floor=1.5, gain=0.5)) > 0


def test_long_strip(gpu):
    """8192 x 32, 4 scans, spread range 4: 32 tiles of 256 rows; strong cells at the plane's edges, at
    rows 2047/2048 and 4095/4096 and at tile seams, each detected, and the 4-row halo on both sides of every
    seam exact."""
    nr, nd, nf = 8192, 32, 4
    rows_per_tile = 8192 // nd
    maps = rayleigh(nf, nr, nd, 7).copy()
    rows = [0, 2047, 2048, 4095, 4096, 8191, rows_per_tile - 1, rows_per_tile, 5 * rows_per_tile - 1, 5 * rows_per_tile,
            31 * rows_per_tile - 1, 31 * rows_per_tile]
    for r in rows:
        for d in (0, 17, nd - 1):
            maps[nf - 1, r, d] = 60.0
    want = check(maps, "strip", alpha=4.0, warmup=2, spread=(4, 1))
    assert {(r, d) for r in rows for d in (0, 17, nd - 1)} <= cells_of(want, nf - 1)
    check(maps, "strip dense", alpha=1.0, warmup=2, spread=(4, 1))


def test_streams_under_the_beamformer(gpu):
    """4 rx, 3 beams, 4 frames of 64 x 64: 12 maps, stream = frame % 3.  The result on the GPU's own maps
    equals three single-stream references interleaved."""
    nr, nd, nrx, nb, nf = 64, 64, 4, 3, 4
    cube = np.ascontiguousarray(synth.frames(nf, nr, nd, nrx, "two_targets", seed=40))
    kw = dict(alpha=1.5, warmup=1)
    with RadarCore(N_RANGE=nr, N_DOPPLER=nd, N_RX=nrx, cfar="none", max_frames=nf) as core, \
            BeamFormer(nr, nd, nrx, steering_weights(nrx, [-0.25, 0.0, 0.25])) as bf, \
            ClutterMap(nr, nd, n_streams=nb, max_frames=nf * nb, **kw) as cm:
        dc = DeviceBuffer(cube.nbytes)
        dc.upload(cube)
        ds = DeviceBuffer(nf * bf.spec_frame_bytes())
        dm = DeviceBuffer(nf * bf.maps_frame_bytes())
        core.range_ct(dc, ds, nf)
        bf.enqueue(ds, nf, dm)
        maps = dm.download(np.float32, (nf * nb, nr, nd))
        got = cm.detect(dm)
        gp, ga = cm.get_state()
        for b in (dc, ds, dm):
            b.free()
    parts, planes = [], []
    for b in range(nb):
        d, p, a = R.detect(maps[b::nb], **kw)
        d["frame"] = d["frame"] * nb + b
        parts.append(d)
        planes.append(p[0])
        assert a.tolist() == [nf]
    want = np.sort(np.concatenate(parts), order=["frame", "range", "doppler"])
    assert len(want) > 0 and got.tobytes() == want.tobytes()
    assert got.tobytes() == R.detect(maps, n_streams=nb, **kw)[0].tobytes()
    assert ga.tolist() == [nf] * nb and gp.tobytes() == np.stack(planes).tobytes()


@pytest.mark.parametrize("nd", [64, 1024])
def test_persistent_loops(gpu, nd):
    """256 x 64 (2 tiles per plane) and 256 x 1024 (32), 2 streams, 3 scans each, under 1, 2 and 5 workgroups
    and the built-in grid: identical bytes."""
    maps = rayleigh(6, 256, nd, 31 + nd)
    kw = dict(n_streams=2, alpha=1.5, warmup=1, spread=(2, 1))
    want, planes, ages = R.detect(maps, **kw)
    assert len(want) > 0
    for grid in (1, 2, 5, 0):
        with ClutterMap(256, nd, max_frames=6, **kw) as cm:
            cm.set_grid_for_test(grid)
            got, st = run(cm, maps)
            assert st.tolist() == [len(want), 0, 0, 0] and got.tobytes() == want.tobytes(), grid
            same_state(cm, planes, ages)


def scan_rounds_maps():
    """129 scans of 64 x 1024 (8 tiles of 8 rows per plane, 1032 tiles): Rayleigh noise, and from scan 1 on
    1 + (f + 3 t) % 5 cells of 1000 in tile t of scan f, at cells that move with f, so that every tile
    after the first scan detects and the counts differ from tile to tile."""
    nf, nr, nd = 129, 64, 1024
    maps = np.random.default_rng(61).rayleigh(1.0, (nf, nr, nd)).astype(np.float32)
    for f in range(1, nf):
        for t in range(8):
            for j in range(1 + (f + 3 * t) % 5):
                maps[f, 8 * t + 1 + j, (37 * f + 101 * j + 7 * t) % nd] = 1000.0
    return maps


def test_scan_beyond_its_first_round(gpu):
    """1032 tiles: k_cmap_scan (det_sink.hpp tile_offsets_scan) takes a second round of 1024 tiles, and
    tile 1024's offset is the first round's total.  Per-tile counts unequal and, past the first scan
    (age 0 detects nothing), non-zero: a wrong carry or offset moves records.  The built-in grid, and 3
    workgroups, each reading offsets of both rounds."""
    maps = scan_rounds_maps()
    nf, nr, nd = maps.shape
    kw = dict(warmup=1)
    want, planes, ages = R.detect(maps, **kw)
    per_tile = np.bincount(want["frame"].astype(np.int64) * 8 + want["range"] // 8, minlength=nf * 8)
    assert len(per_tile) == 1032 and per_tile[8:].min() >= 1 and len(set(per_tile[8:].tolist())) > 1
    for grid in (0, 3):
        with ClutterMap(nr, nd, max_frames=nf, **kw) as cm:
            cm.set_grid_for_test(grid)
            got, st = run(cm, maps, det_cap=len(want) + 8)
            assert st.tolist() == [len(want), 0, 0, 0] and got.tobytes() == want.tobytes(), grid
            same_state(cm, planes, ages)


def test_capacity(gpu):
    """det_cap at half the count, then 0 with a NULL list: the first records only, the full count, and
    the state advancing as if nothing were short.  ClutterMap.detect with a short first capacity returns
    the full list and advances the state exactly once."""
    maps = rayleigh(6, 64, 32, 41)
    kw = dict(alpha=1.0, warmup=2)
    want, planes, ages = R.detect(maps, **kw)
    half = len(want) // 2
    assert half > 100
    with ClutterMap(64, 32, max_frames=6, **kw) as cm:
        got, st = run(cm, maps, det_cap=half)
        assert st.tolist() == [len(want), 0, 0, 0] and got.tobytes() == want[:half].tobytes()
        same_state(cm, planes, ages)
        cm.reset()
        got, st = run(cm, maps, det_cap=0, null_dets=True)
        assert st.tolist() == [len(want), 0, 0, 0] and len(got) == 0
        same_state(cm, planes, ages)
        cm.reset()
        assert cm.detect(maps, det_cap=16).tobytes() == want.tobytes()      # grows from word [0] and reruns once
        same_state(cm, planes, ages)
        more, planes2, ages2 = R.detect(maps[:3], state=(planes, ages), **kw)
        assert cm.detect(maps[:3], det_cap=1).tobytes() == more.tobytes() and ages2.tolist() == [9]
        same_state(cm, planes2, ages2)


def test_state_calls(gpu):
    """reset between two calls on one stream, without a synchronisation between them; get_state then
    set_state into a fresh object continues identically; ages saturate at 0xFFFFFFFF."""
    maps = rayleigh(8, 64, 32, 51)
    kw = dict(alpha=1.3, warmup=2)
    hip = Hip()
    with ClutterMap(64, 32, max_frames=4, **kw) as cm, ClutterMap(64, 32, max_frames=4, **kw) as fresh:
        s = hip.stream()
        dm = DeviceBuffer(maps.nbytes)
        dm.upload(maps)
        dd, dn = DeviceBuffer(4 * 64 * 32 * 16), DeviceBuffer(16)
        try:
            cm.enqueue(dm, 4, dd, 4 * 64 * 32, dn, stream=s.value)
            cm.reset(stream=s.value)
            cm.enqueue(dm.ptr + 4 * 64 * 32 * 4, 4, dd, 4 * 64 * 32, dn, stream=s.value)
            hip.ok(hip.lib.hipStreamSynchronize(s))
            want, planes, ages = R.detect(maps[4:], **kw)             # as on a fresh map
            st = dn.download(np.uint32, (4,))
            assert st.tolist() == [len(want), 0, 0, 0] and len(want) > 0
            assert dd.download(DET_DTYPE, (len(want),)).tobytes() == want.tobytes()
            same_state(cm, planes, ages)
        finally:
            hip.lib.hipStreamDestroy(s)
            for b in (dm, dd, dn):
                b.free()
        # a checkpoint: the fresh object continues as the first one does
        fresh.set_state(*cm.get_state())
        nxt, planes2, ages2 = R.detect(maps[:3], state=(planes, ages), **kw)
        for obj in (cm, fresh):
            got, st = run(obj, maps[:3])
            assert st[0] == len(nxt) > 0 and got.tobytes() == nxt.tobytes()
            same_state(obj, planes2, ages2)
        # planes without ages keep the ages
        fresh.set_state(planes)
        same_state(fresh, planes, ages2)
        # saturation: 0xFFFFFFFE + 3 scans, and 0xFFFFFFFF
        for a0 in (AGE_MAX - 1, AGE_MAX):
            start = (planes, np.array([a0], np.uint32))
            cm.set_state(*start)
            w, p, a = R.detect(maps[:3], state=start, **kw)
            got, st = run(cm, maps[:3])
            assert a.tolist() == [AGE_MAX] and st[0] == len(w) > 0 and got.tobytes() == w.tobytes()
            same_state(cm, p, a)
        lib = L.load()
        assert lib.fmcw_cmap_set_state(cm._h, None, 16, None) == L.FMCW_EINVAL
        assert b"planes_dev" in lib.fmcw_last_error()
        assert lib.fmcw_cmap_get_state(cm._h, None, None, None) == L.FMCW_EINVAL


def test_graph_replay_after_the_map(gpu):
    """fmcw_enqueue (cfar none, 256 x 64, 2 frames) and fmcw_cmap_enqueue captured once on one stream and
    replayed four times on different cubes, with one direct call between the second and third replay: the
    state advances at every replay, so every list and the final state are the reference's over the GPU's
    own maps in the same order."""
    nr, nd, nf = 256, 64, 2
    recipes = [("two_targets", 71), ("random_target", 72), ("two_targets", 73), ("random_target", 74), ("two_targets", 75)]
    cubes = [np.ascontiguousarray(synth.frames(nf, nr, nd, 1, rec, seed=seed)) for rec, seed in recipes]
    kw = dict(alpha=1.5, warmup=1)
    cap = nf * nr * nd
    hip = Hip()
    with RadarCore(N_RANGE=nr, N_DOPPLER=nd, cfar="none", max_frames=nf) as core, \
            ClutterMap(nr, nd, max_frames=nf, **kw) as cm:
        dc, dm = DeviceBuffer(cubes[0].nbytes), DeviceBuffer(nf * nr * nd * 4)
        dd, dn = DeviceBuffer(cap * 16), DeviceBuffer(16)

        def calls(s):
            core.enqueue(dc, nf, dm, stream=s.value)
            cm.enqueue(dm, nf, dd, cap, dn, stream=s.value)

        state = [None]
        counts = []

        def result():
            maps = dm.download(np.float32, (nf, nr, nd))
            st = dn.download(np.uint32, (4,))
            want, planes, ages = R.detect(maps, state=state[0], **kw)
            state[0] = (planes, ages)
            assert st.tolist() == [len(want), 0, 0, 0]
            assert dd.download(DET_DTYPE, (len(want),)).tobytes() == want.tobytes()
            counts.append(len(want))
        try:
            with hip.graph(calls) as (exe, s):
                for i, cube in enumerate(cubes):
                    dc.upload(cube)
                    dn.upload(np.full(16, SENTINEL, np.uint8))
                    if i == 2:
                        calls(s)                                  # a direct call between the replays
                        hip.ok(hip.lib.hipStreamSynchronize(s))
                    else:
                        hip.replay(exe, s)
                    result()
                assert counts[0] > 0 and min(counts[1:]) > 0      # the first call's scan 0 only initialises
                assert state[0][1].tolist() == [2 * len(cubes)]
                same_state(cm, *state[0])
        finally:
            for b in (dc, dm, dd, dn):
                b.free()


def test_chain_to_plots(gpu):
    """A target that appears after the warm-up at 256 x 64: the list goes through the plot extractor, which
    needs it strictly increasing in (frame, range, doppler), unchanged, and gives one plot at the target."""
    nr, nd, nf = 256, 64, 4
    maps = rayleigh(nf, nr, nd, 61).copy()
    maps[nf - 1, 100:103, 20:23] = 30.0
    maps[nf - 1, 101, 21] = 50.0
    with ClutterMap(nr, nd, warmup=3, max_frames=nf) as cm:
        dets = cm.detect(maps)
    assert dets.tobytes() == R.detect(maps, warmup=3)[0].tobytes()
    assert {(r, d) for r in (100, 101, 102) for d in (20, 21, 22)} <= cells_of(dets, nf - 1)
    with PlotExtractor(nr, nd, win=(4, 4), max_dets=len(dets)) as px:
        plots = px.extract(dets)
    near = plots[(plots["frame"] == nf - 1) & (np.abs(plots["range"].astype(int) - 101) <= 4) &
                 (np.abs(plots["doppler"].astype(int) - 21) <= 4)]
    assert len(near) == 1 and (int(near[0]["range"]), int(near[0]["doppler"])) == (101, 21), near
    assert int(near[0]["n_cells"]) >= 9


def test_input_conventions(gpu):
    """Negative cells and -0.0 enter as +0: the signed maps give what the clamped maps give."""
    maps = rayleigh(5, 64, 32, 71).copy()
    rng = np.random.default_rng(72)
    neg = rng.random(maps.shape) < 0.2
    maps[neg] = -maps[neg]
    maps[rng.random(maps.shape) < 0.05] = -0.0
    kw = dict(alpha=1.0, warmup=2, floor=0.1)
    want = check(maps, "signed", **kw)
    assert len(want) > 0 and np.all(want["mag"] > 0)
    assert check(R.nonneg(maps), "clamped", **kw).tobytes() == want.tobytes()
    _, planes, _ = R.detect(maps, **kw)
    assert not np.signbit(planes).any()


def test_zero_frames_and_bad_calls(gpu):
    maps = rayleigh(3, 64, 32, 81)
    kw = dict(alpha=1.0, warmup=1)
    with ClutterMap(64, 32, n_streams=3, max_frames=6, **kw) as cm:
        want, planes, ages = R.detect(maps, n_streams=3, **kw)
        run(cm, maps)
        got, st = run(cm, np.zeros((0, 64, 32), np.float32), det_cap=4)
        assert st.tolist() == [0, 0, 0, 0] and len(got) == 0
        same_state(cm, planes, ages)                                  # zero frames leave the state alone
        lib = L.load()
        dn = DeviceBuffer(16)
        dn.upload(np.full(16, SENTINEL, np.uint8))
        assert lib.fmcw_cmap_enqueue(cm._h, None, 0, None, 0, dn.ptr, None) == L.FMCW_OK
        assert dn.download(np.uint32, (4,)).tolist() == [0, 0, 0, 0]
        assert lib.fmcw_cmap_enqueue(cm._h, None, 3, None, 0, dn.ptr, None) == L.FMCW_EINVAL
        assert lib.fmcw_cmap_enqueue(cm._h, dn.ptr, 4, None, 0, dn.ptr, None) == L.FMCW_EINVAL
        assert b"multiple of n_streams" in lib.fmcw_last_error()
        assert lib.fmcw_cmap_enqueue(cm._h, dn.ptr, 9, None, 0, dn.ptr, None) == L.FMCW_EINVAL
        assert b"max_frames" in lib.fmcw_last_error()
        assert lib.fmcw_cmap_enqueue(cm._h, dn.ptr + 4, 3, None, 0, dn.ptr, None) == L.FMCW_EINVAL
        assert b"16-byte" in lib.fmcw_last_error()
        assert lib.fmcw_cmap_enqueue(cm._h, dn.ptr, 3, dn.ptr + 4, 1, dn.ptr, None) == L.FMCW_EINVAL
        assert b"16-byte" in lib.fmcw_last_error()
        assert lib.fmcw_cmap_get_state(cm._h, dn.ptr + 4, None, None) == L.FMCW_EINVAL
        same_state(cm, planes, ages)                                  # nor does a refused call
        dn.free()
