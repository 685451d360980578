"""The cell-averaging detector on the GPU (fmcw_cacfar_* of libfmcw.so on gfx950 through the C-ABI).
Lists and status words are compared bit for bit with tests/cacfar_ref.py (the header's specification in
NumPy float32).  Every run writes into sentinel-filled buffers and checks the records after the list.

Shapes are the smallest at which each mechanism can go wrong: 64 x 32 for the modes, the dense list and
the window matrix (one tile per frame, two steps of 32 rows); n_range 64 with every n_doppler 32 .. 1024
(32 .. 1 rows per step, the Doppler wrap at both ends of a row, the first and last tested rows and the
rows just outside them); 8192 x 32 for a strip of 2048 rows (64 steps through the rings); 5 frames of
256 x 64 under 1 and 2 workgroups for the persistent loop.
"""
import numpy as np
import pytest

import cacfar_ref as R
from fmcw import DET_DTYPE, BeamFormer, CaCfar, DeviceBuffer, PlotExtractor, RadarCore, steering_weights, synth
from fmcw import _lib as L
from gpu_support import SENTINEL, Hip, rayleigh, run_map_detector

pytestmark = pytest.mark.gpu

CANARY = 8          # sentinel records kept after the list
DEFAULT = ((4, 4), (1, 2))


def run(det, maps, det_cap=None, null_dets=False):
    """One fmcw_cacfar_enqueue on host maps: (the records written, the four status words), after
    checking that every record from min(found, det_cap) on kept the sentinel."""
    return run_map_detector(det, maps, det_cap, null_dets, canary=CANARY)


def check(maps, mode="ca", ref=DEFAULT[0], guard=DEFAULT[1], alpha=4.0, label=""):
    maps = np.asarray(maps, np.float32)
    nf, nr, nd = maps.shape
    want = R.detect(maps, mode, ref, guard, alpha)
    with CaCfar(nr, nd, mode=mode, ref=ref, guard=guard, alpha=alpha, max_frames=nf) as det:
        got, st = run(det, maps)
    print(f"\n{label or mode} {nr}x{nd}x{nf} {ref}/{guard} alpha {alpha}: {len(want)} detections "
          f"({len(want) / max((nr - 2 * (ref[0] + guard[0])) * nd * nf, 1):.3f} of the tested cells)")
    assert st.tolist() == [len(want), 0, 0, 0]
    assert got.tobytes() == want.tobytes()
    return want


@pytest.mark.parametrize("mode", R.MODES)
def test_modes_on_the_golden_map(gpu, golden, mode):
    m = np.load(golden / "tb_cfar2d.npz")["map"].astype(np.float32)[None]
    want = check(m, mode, (3, 2), (1, 1), 4.0)
    assert len(want) == 18


def test_dense_list_and_short_capacity(gpu):
    """3 frames of 64 x 32 Rayleigh noise at alpha 1 (about 45 % of the tested cells): the full list;
    det_cap = half the count; det_cap 0 with a NULL list."""
    maps = rayleigh(3, 64, 32, 11)
    want = check(maps, "ca", alpha=1.0)
    assert 0.3 < len(want) / (54 * 32 * 3) < 0.6
    half = len(want) // 2
    with CaCfar(64, 32, alpha=1.0, max_frames=3) as det:
        got, st = run(det, maps, det_cap=half)
        assert st.tolist() == [len(want), 0, 0, 0] and got.tobytes() == want[:half].tobytes()
        got, st = run(det, maps, det_cap=0, null_dets=True)
        assert st.tolist() == [len(want), 0, 0, 0] and len(got) == 0
        got, st = run(det, maps[:2])                                  # fewer frames than max_frames
        assert got.tobytes() == want[want["frame"] < 2].tobytes()
        assert det.detect(maps, det_cap=16).tobytes() == want.tobytes()   # grows from word [0] and reruns


def strong_cells(nr, nd, hr):
    """Rows: the first and last tested ones and the rows just outside them; columns: both ends of the
    circular Doppler axis and one in the middle."""
    return [(r, d) for r in (hr - 1, hr, nr - 1 - hr, nr - hr) for d in (0, nd // 2 + 3, nd - 1)]


@pytest.mark.parametrize("nd", [32, 64, 128, 256, 512, 1024])
def test_every_doppler_size(gpu, nd):
    nr, hr = 64, 5
    maps = rayleigh(2, nr, nd, 100 + nd).copy()
    cells = strong_cells(nr, nd, hr)
    for f in range(2):
        for r, d in cells:
            maps[f, r, d] = 40.0 + f
    for mode in R.MODES:
        want = check(maps, mode)
        seen = set(zip(want["frame"].tolist(), want["range"].tolist(), want["doppler"].tolist()))
        for f in range(2):
            for r, d in cells:
                assert ((f, r, d) in seen) == (hr <= r < nr - hr), (mode, f, r, d)
        assert want["range"].min() >= hr and want["range"].max() < nr - hr
    check(maps, "ca", alpha=1.0, label="ca dense")     # about 45 % of the cells: their thresholds, bit for bit


def test_long_strip(gpu):
    """8192 x 32: tiles of 2048 rows, 64 steps each, the rings wrapped many times; strong cells at the
    tile seams and the tested edges."""
    nr, nd, hr = 8192, 32, 5
    maps = rayleigh(1, nr, nd, 7).copy()
    for r in (hr - 1, hr, 2047, 2048, 4095, 4096, nr - 1 - hr, nr - hr):
        for d in (0, 17, nd - 1):
            maps[0, r, d] = 50.0
    for mode, alpha in (("ca", 4.0), ("so", 1.0)):
        want = check(maps, mode, alpha=alpha)
        rows = set(want["range"][want["mag"] == 50.0].tolist())
        assert rows == {hr, 2047, 2048, 4095, 4096, nr - 1 - hr}


@pytest.mark.parametrize("ref,guard", [((4, 4), (1, 2)), ((0, 8), (0, 2)), ((8, 0), (0, 0)), ((1, 1), (0, 0)),
                                       ((8, 8), (4, 4))])
def test_window_matrix(gpu, ref, guard):
    """Window (Rr, Gr, Rd, Gd) = (4,1,4,2), (0,0,8,2), (8,0,0,0), (1,0,1,0), (8,4,8,4) at 64 x 32, alpha 1."""
    maps = rayleigh(2, 64, 32, 21)
    for mode in R.MODES:
        want = check(maps, mode, ref, guard, 1.0)
        assert len(want) > 0


def test_persistent_loops(gpu):
    """5 frames of 256 x 64 (a frame is one tile at this size): 1 and 2 workgroups walk 5 and 3 tiles
    and give the built-in grid's bytes."""
    maps = rayleigh(5, 256, 64, 31)
    want = R.detect(maps, "go", alpha=1.5)
    with CaCfar(256, 64, mode="go", alpha=1.5, max_frames=5) as det:
        base, st = run(det, maps)
        assert st.tolist() == [len(want), 0, 0, 0] and base.tobytes() == want.tobytes()
        for grid in (1, 2, 0):
            det.set_grid_for_test(grid)
            got, st2 = run(det, maps)
            assert got.tobytes() == base.tobytes() and st2.tolist() == st.tolist(), grid


def test_persistent_loops_with_several_tiles_per_frame(gpu):
    """3 frames of 256 x 1024: tiles of 64 rows, 4 per frame, 12 in all, under 1 and 5 workgroups."""
    maps = rayleigh(3, 256, 1024, 32)
    want = R.detect(maps, "ca", alpha=3.0)
    with CaCfar(256, 1024, alpha=3.0, max_frames=3) as det:
        for grid in (0, 1, 5):
            det.set_grid_for_test(grid)
            got, st = run(det, maps)
            assert st.tolist() == [len(want), 0, 0, 0] and got.tobytes() == want.tobytes(), grid


def scan_rounds_maps():
    """1025 frames of 64 x 32 (one tile per frame): Rayleigh noise and 1 + f % 7 cells of 60 in frame f,
    6 rows apart (outside each other's window of +-5 rows), so that no tile is empty and the counts
    differ from tile to tile."""
    nf, nr, nd = 1025, 64, 32
    maps = np.random.default_rng(51).rayleigh(1.0, (nf, nr, nd)).astype(np.float32)
    for f in range(nf):
        for j in range(1 + f % 7):
            maps[f, 8 + 6 * j, (5 * j + f) % nd] = 60.0
    return maps


def test_scan_beyond_its_first_round(gpu):
    """1025 tiles: k_cacfar_scan (det_sink.hpp tile_offsets_scan) takes a second round of 1024 tiles, and
    tile 1024's offset is the first round's total.  Unequal, non-zero counts per tile: a wrong carry or
    offset moves records.  The built-in grid, and 3 workgroups, each reading offsets of both rounds."""
    maps = scan_rounds_maps()
    nf, nr, nd = maps.shape
    want = R.detect(maps)
    per_tile = np.bincount(want["frame"], minlength=nf)          # one tile per frame at 64 x 32
    assert len(per_tile) == 1025 and per_tile.min() >= 1 and len(set(per_tile.tolist())) > 1
    with CaCfar(nr, nd, max_frames=nf) as det:
        for grid in (0, 3):
            det.set_grid_for_test(grid)
            got, st = run(det, maps, det_cap=len(want) + 8)
            assert st.tolist() == [len(want), 0, 0, 0] and got.tobytes() == want.tobytes(), grid


def test_input_conventions(gpu):
    """Negative cells and -0.0 enter as +0; +Inf cells follow IEEE arithmetic: the reference on the
    same map (which clamps as the header says)."""
    maps = rayleigh(2, 64, 32, 41).copy()
    rng = np.random.default_rng(42)
    neg = rng.random(maps.shape) < 0.2
    maps[neg] = -maps[neg]
    maps[rng.random(maps.shape) < 0.05] = -0.0
    for mode in R.MODES:
        want = check(maps, mode, alpha=1.0, label=f"{mode} signed")
        assert np.all(want["mag"] > 0)
        clamped = check(R.nonneg(maps), mode, alpha=1.0, label=f"{mode} clamped")
        assert want.tobytes() == clamped.tobytes()
    inf = rayleigh(1, 64, 32, 43).copy()
    inf[0, 20, 5] = inf[0, 40, 31] = inf[0, 41, 0] = np.inf
    for mode in R.MODES:
        want = check(inf, mode, alpha=1.0, label=f"{mode} inf")
        assert np.isinf(want["mag"]).sum() == 3 and np.all(np.isfinite(want["threshold"]))


def test_graph_replay_after_the_map(gpu):
    """fmcw_enqueue (cfar none, 256 x 64, 2 frames) and fmcw_cacfar_enqueue captured once on one stream,
    replayed on two cubes with one direct call between the replays: every list is the reference's on
    the GPU's own maps."""
    nr, nd, nf = 256, 64, 2
    cubes = [np.ascontiguousarray(synth.frames(nf, nr, nd, 1, "two_targets", seed=71)),
             np.ascontiguousarray(synth.frames(nf, nr, nd, 1, "random_target", seed=72))]
    cap = nf * nr * nd
    hip = Hip()
    with RadarCore(N_RANGE=nr, N_DOPPLER=nd, cfar="none", max_frames=nf) as core, \
            CaCfar(nr, nd, mode="so", alpha=3.0, max_frames=nf) as det:
        dc, dm = DeviceBuffer(cubes[0].nbytes), DeviceBuffer(nf * nr * nd * 4)
        dd, dn = DeviceBuffer(cap * 16), DeviceBuffer(16)

        def calls(s):
            core.enqueue(dc, nf, dm, stream=s.value)
            det.enqueue(dm, nf, dd, cap, dn, stream=s.value)

        def result():
            maps = dm.download(np.float32, (nf, nr, nd))
            st = dn.download(np.uint32, (4,))
            want = R.detect(maps, "so", alpha=3.0)
            assert st.tolist() == [len(want), 0, 0, 0] and len(want) > 0
            assert dd.download(DET_DTYPE, (len(want),)).tobytes() == want.tobytes()
            return want.tobytes()
        try:
            with hip.graph(calls) as (exe, s):
                dc.upload(cubes[0])
                hip.replay(exe, s)
                first = result()
                dc.upload(cubes[1])
                calls(s)                                      # a direct call between the replays
                hip.ok(hip.lib.hipStreamSynchronize(s))
                direct = result()
                dn.upload(np.zeros(4, np.uint32))
                hip.replay(exe, s)
                assert result() == direct != first
        finally:
            for b in (dc, dm, dd, dn):
                b.free()


def test_chain_to_plots(gpu):
    """two_targets at 256 x 64 through the path (no CFAR), the detector and the plot extractor: both
    targets are detected, and the extractor, which needs a list strictly increasing in (frame, range,
    doppler), gives exactly one plot in each target's neighbourhood, at the target's cell."""
    nr, nd = 256, 64
    cube = synth.frames(1, nr, nd, 1, "two_targets", seed=5)
    with RadarCore(N_RANGE=nr, N_DOPPLER=nd, cfar="none", max_frames=1) as core:
        maps = core.process(cube).rd_map
    with CaCfar(nr, nd) as det:
        dets = det.detect(maps)
    assert dets.tobytes() == R.detect(maps).tobytes()
    cells = set(zip(dets["range"].tolist(), dets["doppler"].tolist()))
    targets = [(25, 5), (125, 54)]
    assert all(t in cells for t in targets)
    with PlotExtractor(nr, nd, win=(4, 4), max_dets=len(dets)) as px:
        plots = px.extract(dets)
    for r, d in targets:
        dd = (plots["doppler"].astype(int) - d + nd // 2) % nd - nd // 2
        near = plots[(np.abs(plots["range"].astype(int) - r) <= 4) & (np.abs(dd) <= 4)]
        assert len(near) == 1 and (int(near[0]["range"]), int(near[0]["doppler"])) == (r, d), near


def test_chain_under_the_beamformer(gpu):
    """4 rx, 3 beams, 2 frames of 64 x 64: the detector on the n_frames * n_beams maps, exact against
    the reference on those maps; frame % 3 is the beam."""
    nr, nd, nrx, nb, nf = 64, 64, 4, 3, 2
    cube = np.ascontiguousarray(synth.frames(nf, nr, nd, nrx, "two_targets", seed=40))
    with RadarCore(N_RANGE=nr, N_DOPPLER=nd, N_RX=nrx, cfar="none", max_frames=nf) as core, \
            BeamFormer(nr, nd, nrx, steering_weights(nrx, [-0.25, 0.0, 0.25])) as bf, \
            CaCfar(nr, nd, mode="go", max_frames=nf * nb) as det:
        dc = DeviceBuffer(cube.nbytes)
        dc.upload(cube)
        ds = DeviceBuffer(nf * bf.spec_frame_bytes())
        dm = DeviceBuffer(nf * bf.maps_frame_bytes())
        core.range_ct(dc, ds, nf)
        bf.enqueue(ds, nf, dm)
        maps = dm.download(np.float32, (nf * nb, nr, nd))
        got = det.detect(dm)
        for b in (dc, ds, dm):
            b.free()
    want = R.detect(maps, "go")
    assert got.tobytes() == want.tobytes() and len(want) > 0
    assert set((want["frame"] // nb).tolist()) == {0, 1}
    at = want[(want["range"] == 100 * nr // 1024) & (want["doppler"] == 5)]
    assert len(at) and all(int(f) % nb == 2 for f in at["frame"][at["mag"] == at["mag"].max()])   # rx_phase 0.25


def test_zero_frames(gpu):
    with CaCfar(64, 32) as det:
        got, st = run(det, np.zeros((0, 64, 32), np.float32), det_cap=4)
        assert st.tolist() == [0, 0, 0, 0] and len(got) == 0
        lib = L.load()
        dn = DeviceBuffer(16)
        dn.upload(np.full(16, SENTINEL, np.uint8))
        assert lib.fmcw_cacfar_enqueue(det._h, None, 0, None, 0, dn.ptr, None) == L.FMCW_OK
        assert dn.download(np.uint32, (4,)).tolist() == [0, 0, 0, 0]
        assert lib.fmcw_cacfar_enqueue(det._h, None, 1, None, 0, dn.ptr, None) == L.FMCW_EINVAL
        assert lib.fmcw_cacfar_enqueue(det._h, dn.ptr, 2, None, 0, dn.ptr, None) == L.FMCW_EINVAL
        assert b"max_frames" in lib.fmcw_last_error()
        assert lib.fmcw_cacfar_enqueue(det._h, dn.ptr, 1, dn.ptr + 4, 1, dn.ptr, None) == L.FMCW_EINVAL
        assert b"16-byte" in lib.fmcw_last_error()
        dn.free()
