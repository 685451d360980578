"""Coherent beamforming on the GPU (fmcw_beams_* of libfmcw.so on gfx950 through the C-ABI), every
case against tests/beams_ref.py (the specification in fp64 NumPy) run on the GPU's own fmcw_range_ct
output downloaded to the host.  The tolerance is beams_ref.assert_maps_match's (the project's map
tolerance at the scale before cancellation); every comparison prints the worst fraction of each bound.

Shapes: n_range 64 with every n_doppler 32 .. 1024 (each its own kernel instantiation and last-pass
radix; 2 .. 64 wave tiles per frame); n_rx 1..4; 1, 3 and 8 beams; MTI off, 2- and 3-pulse; Hamming
and no window; 3 frames (two_targets at rx_phase 0.25 / -0.125, random_target at 0.25, two_targets
again), so that at n_doppler 32 the 6 wave tiles are no multiple of a workgroup's 4.

On those scenes (a few tones over weak noise) nearly every map cell lies below 1e-4 of the map's largest
scale, where a zero or another row's value passes (tests/test_beams_host.py measures it).  The
full-scale cases run on beams_ref.full_scale_spec instead, a white Gaussian spectrum from the host on
which the same bounds hold every cell: every n_doppler x n_rx 1, 4 x MTI, n_rx 64 and n_beams 64, and
the capped grids.  run() also fails on any map word that still holds the sentinel the buffer was
filled with (as a float it is -2.9e-16, a zero for the tolerance).
"""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

import fmcw_oracle as O
from fmcw import DET_DTYPE, BeamFormer, DeviceBuffer, RadarCore, cli, formats, steering_weights, synth
from fmcw import _lib as L
import beams_ref as BR
from beams_ref import assert_maps_match, beams_ref
from gpu_support import SENTINEL, Hip, range_ct_spectrum as range_ct, run_beams as run

pytestmark = pytest.mark.gpu

TAIL = 4096       # sentinel bytes in the buffers of the tests of calls that must write nothing
NF = 3
NR = 64
DOPPLERS = [32, 64, 128, 256, 512, 1024]
MTIS = [0, 2, 3]
PHASES = [0.25, -0.125]     # two_targets: the first target a quarter cycle per element


def three_frame_cube(nr, nc, nrx, seed=40):
    return np.ascontiguousarray(np.concatenate([
        synth.frames(1, nr, nc, nrx, "two_targets", seed=seed, rx_phase=PHASES),
        synth.frames(1, nr, nc, nrx, "random_target", seed=seed + 1, rx_phase=0.25),
        synth.frames(1, nr, nc, nrx, "two_targets", seed=seed + 2, rx_phase=PHASES)]))


@functools.lru_cache(maxsize=None)
def scene(nc, nrx, nr=NR):
    cube = three_frame_cube(nr, nc, nrx)
    spec = range_ct(cube, nr, nc, nrx)
    assert np.any(spec[NF - 1])
    for a in (cube, spec):
        a.setflags(write=False)
    return SimpleNamespace(cube=cube, spec=spec, nr=nr, nc=nc, nrx=nrx)


def check(sc, weights, win, mti, label):
    ref, S = beams_ref(sc.spec, weights, win=win, mti=mti)
    with BeamFormer(sc.nr, sc.nc, sc.nrx, weights, window=win, mti=mti) as bf:
        got = run(bf, sc.spec)
    assert_maps_match(got, ref, S, label=label)
    return got


def case_weights(nrx, nb, seed):
    """(steering weights over (-0.5, 0.5) with 0.25 among them, a random complex matrix)."""
    nus = 0.25 + np.arange(nb) / nb
    rng = np.random.default_rng(seed)
    rnd = (rng.standard_normal((nb, nrx)) + 1j * rng.standard_normal((nb, nrx))).astype(np.complex64)
    return steering_weights(nrx, (nus + 0.5) % 1.0 - 0.5), rnd


@pytest.mark.parametrize("mti", MTIS)
@pytest.mark.parametrize("nrx", [1, 2, 3, 4])
@pytest.mark.parametrize("nc", DOPPLERS)
def test_against_reference(gpu, nc, nrx, mti):
    """Steering weights and one random complex matrix (it catches a transposed or conjugated weight)
    per case; the beam count (1, 3, 8) and the window alternate over the matrix so that each meets
    every n_doppler, n_rx and MTI mode."""
    i, mi = DOPPLERS.index(nc), MTIS.index(mti)
    nb = (1, 3, 8)[(i + nrx + mi) % 3]
    win = ("hamming", "none")[(i + mi + nrx // 2) % 2]
    sc = scene(nc, nrx)
    steer, rnd = case_weights(nrx, nb, seed=1000 * nc + 10 * nrx + mti)
    label = f"{NR}x{nc} rx{nrx} beams{nb} mti{mti} {win}"
    check(sc, steer, win, mti, label + " steering")
    check(sc, rnd, win, mti, label + " random")


@pytest.mark.parametrize("nb", [1, 3, 8])
@pytest.mark.parametrize("win", ["hamming", "none"])
@pytest.mark.parametrize("mti", MTIS)
def test_window_mti_and_beams_at_one_shape(gpu, win, mti, nb):
    """Every window x MTI x beam count at one shape (the matrix above alternates them)."""
    sc = scene(128, 4)
    check(sc, case_weights(4, nb, seed=7 + nb)[1], win, mti, f"{NR}x128 rx4 beams{nb} mti{mti} {win}")


@pytest.mark.parametrize("win", ["hamming", "none"])
@pytest.mark.parametrize("mti", MTIS)
@pytest.mark.parametrize("nc", [32, 256])
def test_one_channel_unit_weight_is_the_path_map(gpu, nc, mti, win):
    """n_rx = 1, W = [[1]]: RadarCore.process's linear map of the same cube for the same window and
    MTI mode, within the same bound (S is then the reference map itself)."""
    cube = three_frame_cube(NR, nc, 1)
    with RadarCore(N_RANGE=NR, N_DOPPLER=nc, N_RX=1, cfar="none", max_frames=NF, window=win,
                   mti_bypass=mti == 0, NOTCH_MODE=mti or 2) as core:
        path = core.process(cube).rd_map
    spec = range_ct(cube, NR, nc, 1, win)
    with BeamFormer(NR, nc, 1, [[1.0]], window=win, mti=mti) as bf:
        got = run(bf, spec)
    ref, S = beams_ref(spec, [[1.0]], win=win, mti=mti)
    assert_maps_match(got, ref, S, label=f"{NR}x{nc} mti{mti} {win} beam")
    assert_maps_match(path[:, None], ref, S, label=f"{NR}x{nc} mti{mti} {win} path")
    assert_maps_match(got, path[:, None].astype(np.float64), S, label=f"{NR}x{nc} mti{mti} {win} beam vs path")


@pytest.mark.parametrize("nc", [32, 1024])
@pytest.mark.parametrize("nrx", [2, 3, 4])
def test_null_and_main_beam(gpu, nrx, nc):
    """Beams at nu = 0.25 + j / n_rx: at the first target's peak cell (rx_phase 0.25) beam 0 holds the
    maximum over the beams and every other beam at most 1e-2 of it -- on the reference first (which
    alone gives <= 5e-5, tests/test_beams_host.py), then on the GPU."""
    sc = scene(nc, nrx)
    w = steering_weights(nrx, 0.25 + np.arange(nrx) / nrx)
    ref, S = beams_ref(sc.spec, w)
    r, d = 100 * NR // 1024, 5
    with BeamFormer(NR, nc, nrx, w) as bf:
        got = run(bf, sc.spec)
    assert_maps_match(got, ref, S, label=f"{NR}x{nc} rx{nrx} orthogonal beams")
    for f in (0, 2):                                   # the two_targets frames
        for name, m in (("reference", ref), ("gpu", got)):
            cell = m[f, :, r, d].astype(np.float64)
            print(f"\n{name} rx{nrx} {NR}x{nc} frame {f}: other beams / beam 0 = {cell[1:] / cell[0]}")
            assert cell.argmax() == 0 and np.all(cell[1:] <= 1e-2 * cell[0]), (name, f, cell)


@pytest.mark.parametrize("nc,nrx,mti", [(32, 3, 0), (1024, 2, 2), (32, 2, 3), (1024, 4, 0)])
def test_grid_independence(gpu, nc, nrx, mti):
    """1 and 3 workgroups through the hook, then the built-in grid again, on the same object, 3 frames
    and 3 beams: a workgroup then passes several tiles, frames and beams (at 1024, 192 tiles over 12
    waves).  The reference's values, and the same bytes each time."""
    sc = scene(nc, nrx)
    w = case_weights(nrx, 3, seed=nc + nrx)[1]
    ref, S = beams_ref(sc.spec, w, mti=mti)
    with BeamFormer(NR, nc, nrx, w, mti=mti) as bf:
        base = run(bf, sc.spec)
        assert_maps_match(base, ref, S, label=f"{NR}x{nc} rx{nrx} mti{mti} built-in grid")
        for grid in (1, 3, 0):
            bf.set_grid_for_test(grid)
            assert run(bf, sc.spec).tobytes() == base.tobytes(), grid


# ---- the full-scale scene: white Gaussian cells, so that the bounds hold every map cell -------------------
@functools.lru_cache(maxsize=None)
def full_scale(nc, nrx, mti, nb=BR.FS_NB):
    """(spec, weights, win, ref, S) of beams_ref.full_scale_case: a spectrum from the host, no range FFT.
    tests/test_beams_host.py shows on the reference alone that a zero, the neighbouring row and the
    next frame's or beam's map pass in at most 2 % of these cells."""
    spec, w, win = BR.full_scale_case(nc, nrx, mti, nb)
    ref, S = beams_ref(spec, w, win=win, mti=mti)
    for a in (w, ref, S):
        a.setflags(write=False)
    return spec, w, win, ref, S


@pytest.mark.parametrize("mti", BR.FS_MTIS)
@pytest.mark.parametrize("nrx", BR.FS_RXS)
@pytest.mark.parametrize("nc", BR.FS_DOPPLERS)
def test_full_scale_against_reference(gpu, nc, nrx, mti):
    """2 frames, 3 beams of random complex weights, every n_doppler (many rows per wave at 32, one row
    per tile at 1024): a wrong tile-to-row or tile-to-frame mapping, a sum carried over between beams or
    a wrong canceller edge is out of bound wherever it falls."""
    spec, w, win, ref, S = full_scale(nc, nrx, mti)
    with BeamFormer(NR, nc, nrx, w, window=win, mti=mti) as bf:
        got = run(bf, spec)
    assert_maps_match(got, ref, S, label=f"full scale {NR}x{nc} rx{nrx} beams{BR.FS_NB} mti{mti} {win}")


@pytest.mark.parametrize("nrx,nb", BR.FS_LIMITS)
def test_full_scale_at_the_header_limits(gpu, nrx, nb):
    """n_rx 64 and n_beams 64, the largest the header allows, at 64 x 32."""
    spec, w, win, ref, S = full_scale(32, nrx, 0, nb)
    with BeamFormer(NR, 32, nrx, w, window=win) as bf:
        got = run(bf, spec)
    assert_maps_match(got, ref, S, label=f"full scale {NR}x32 rx{nrx} beams{nb} mti0 {win}")


@pytest.mark.parametrize("nc,nrx,mti", [(32, 4, 0), (1024, 1, 2), (32, 1, 3), (1024, 4, 3)])
def test_full_scale_grid_independence(gpu, nc, nrx, mti):
    """1 and 3 workgroups through the hook, then the built-in grid again, on the full-scale scene: a
    workgroup's later tiles, frames and beams are held to the reference in every cell, and not only to
    the first run's bytes."""
    spec, w, win, ref, S = full_scale(nc, nrx, mti)
    with BeamFormer(NR, nc, nrx, w, window=win, mti=mti) as bf:
        base = run(bf, spec)
        assert_maps_match(base, ref, S, label=f"full scale {NR}x{nc} rx{nrx} mti{mti} {win} built-in grid")
        for grid in (1, 3, 0):
            bf.set_grid_for_test(grid)
            got = run(bf, spec)
            assert_maps_match(got, ref, S, label=f"full scale {NR}x{nc} rx{nrx} mti{mti} {win} grid {grid}")
            assert got.tobytes() == base.tobytes(), grid


def test_graph_replay_on_a_second_cube(gpu):
    """fmcw_range_ct and fmcw_beams_enqueue captured once into one graph and replayed twice, a
    different cube uploaded between the replays: each replay matches the reference on that replay's
    own spectrum."""
    nc, nrx, nb = 64, 4, 3
    cubes = [three_frame_cube(NR, nc, nrx, seed=40), three_frame_cube(NR, nc, nrx, seed=60)]
    w = case_weights(nrx, nb, seed=3)[1]
    hip = Hip()
    with RadarCore(N_RANGE=NR, N_DOPPLER=nc, N_RX=nrx, cfar="none", max_frames=NF) as core, \
            BeamFormer(NR, nc, nrx, w) as bf:
        dc = DeviceBuffer(cubes[0].nbytes)
        ds = DeviceBuffer(NF * bf.spec_frame_bytes())
        dm = DeviceBuffer(NF * bf.maps_frame_bytes())

        def calls(s):
            core.range_ct(dc, ds, NF, stream=s.value)
            bf.enqueue(ds, NF, dm, stream=s.value)
        try:
            with hip.graph(calls) as (exe, s):
                seen = []
                for k in (0, 1):
                    dc.upload(cubes[k])
                    hip.replay(exe, s)
                    spec = ds.download(np.complex64, (NF, nrx, NR, nc))
                    got = dm.download(np.float32, (NF, nb, NR, nc))
                    assert_maps_match(got, *beams_ref(spec, w), label=f"replay {k}")
                    seen.append(got.tobytes())
                assert seen[0] != seen[1]
        finally:
            for b in (dc, ds, dm):
                b.free()


def test_chain_to_cfar(gpu):
    """range_ct -> beams -> cfar: 4 rx, 8 beams at (b - 4) / 8, 64 x 64, the core's 1-D OS-CFAR over
    the NF * 8 maps as NF * 8 frames.  The list is bit-exact against the oracle's CFAR on the GPU's
    own maps; frame // 8 and frame % 8 recover frame and beam; the first target's strongest detection
    lies in the beam at nu = 0.25."""
    nc, nrx, nb = 64, 4, 8
    sc = scene(nc, nrx)
    nus = (np.arange(nb) - nb // 2) / nb
    n_maps = NF * nb
    with BeamFormer(NR, nc, nrx, steering_weights(nrx, nus)) as bf, \
            RadarCore(N_RANGE=NR, N_DOPPLER=nc, N_RX=1, cfar="os1d", max_frames=n_maps) as core:
        dspec = DeviceBuffer(sc.spec.nbytes)
        dspec.upload(sc.spec)
        dm = DeviceBuffer(NF * bf.maps_frame_bytes())
        cap = n_maps * NR * nc
        dd, dn = DeviceBuffer(cap * 16), DeviceBuffer(16)
        bf.enqueue(dspec, NF, dm)
        core.cfar(dm, n_maps, dd, cap, dn)
        st = dn.download(np.uint32, (4,))
        maps = dm.download(np.float32, (n_maps, NR, nc))
        dets = dd.download(DET_DTYPE, (int(st[0]),))
        for b in (dspec, dm, dd, dn):
            b.free()
    assert st[1] == 0 and 0 < st[0] <= cap
    want = []
    for m in range(n_maps):
        det, thr = O.cfar_os1d(maps[m], O.Cfar1D())
        want.append(O.detections(det, maps[m], thr, frame=m))
    np.testing.assert_array_equal(dets, np.concatenate(want))
    ref, S = beams_ref(sc.spec, steering_weights(nrx, nus))
    assert_maps_match(maps.reshape(NF, nb, NR, nc), ref, S, label="chain maps")
    frame, beam = dets["frame"] // nb, dets["frame"] % nb
    assert set(frame.tolist()) == set(range(NF)) and beam.max() < nb
    r, d = 100 * NR // 1024, 5
    for f in (0, 2):
        at = (frame == f) & (dets["range"] == r) & (dets["doppler"] == d)
        assert at.any(), f"frame {f}: the first target's peak cell is not detected in any beam"
        best = dets[at][np.argmax(dets["mag"][at])]
        assert nus[int(best["frame"]) % nb] == 0.25, (f, best)
        assert np.array_equal(maps[int(best["frame"]), r, d], best["mag"])


def test_zero_frames_is_a_no_op(gpu):
    lib = L.load()
    with BeamFormer(NR, 32, 2, case_weights(2, 3, seed=1)[0]) as bf:
        dm = DeviceBuffer(TAIL)
        dm.upload(np.full(TAIL, SENTINEL, np.uint8))
        bf.enqueue(dm, 0, dm)
        assert lib.fmcw_beams_enqueue(bf._h, None, 0, None, None) == L.FMCW_OK      # nothing is looked at
        assert np.all(dm.download(np.uint8, (TAIL,)) == SENTINEL)
        assert lib.fmcw_beams_enqueue(bf._h, None, 1, dm.ptr, None) == L.FMCW_EINVAL
        assert lib.fmcw_beams_enqueue(bf._h, dm.ptr, 1, dm.ptr + 4, None) == L.FMCW_EINVAL
        assert b"16-byte" in lib.fmcw_last_error()
        assert np.all(dm.download(np.uint8, (TAIL,)) == SENTINEL)
        dm.free()


def test_form_and_cli(gpu, tmp_path):
    """form() on a host spectrum and on a device one gives enqueue's bytes; --beams 8 on a 4-channel
    .npy writes ADR_beam_detections.txt with the chain's detections and leaves the detection file as it
    is written without it."""
    nc, nrx, nb = 64, 4, 8
    sc = scene(nc, nrx)
    nus = (np.arange(nb) - nb // 2) / nb
    with BeamFormer(NR, nc, nrx, steering_weights(nrx, nus)) as bf:
        maps = run(bf, sc.spec)
        assert bf.form(sc.spec).tobytes() == maps.tobytes()
        ds = DeviceBuffer(sc.spec.nbytes)
        ds.upload(sc.spec)
        assert bf.form(ds).tobytes() == maps.tobytes()
        ds.free()
    np.save(tmp_path / "cube.npy", sc.cube)
    common = [str(tmp_path / "cube.npy"), "--n-range", str(NR), "--n-doppler", str(nc), "--cfar", "os1d"]
    cli.main(common + ["--out-dir", str(tmp_path / "plain")])
    cli.main(common + ["--out-dir", str(tmp_path / "b"), "--beams", str(nb), "--rx-spacing", "0.25"])
    assert sorted(p.name for p in (tmp_path / "plain").iterdir()) == ["ADR_detections.txt"]
    assert sorted(p.name for p in (tmp_path / "b").iterdir()) == ["ADR_beam_detections.txt", "ADR_detections.txt"]
    assert (tmp_path / "b" / "ADR_detections.txt").read_bytes() == (tmp_path / "plain" / "ADR_detections.txt").read_bytes()
    want = []
    for m, mp in enumerate(maps.reshape(NF * nb, NR, nc)):
        det, thr = O.cfar_os1d(mp, O.Cfar1D())
        want.append(O.detections(det, mp, thr, frame=m))
    want = np.concatenate(want)
    got = formats.read_beam_detections(tmp_path / "b" / "ADR_beam_detections.txt")
    assert len(got) == len(want) > 0
    np.testing.assert_array_equal(got[:, 0], want["frame"] // nb)
    np.testing.assert_array_equal(got[:, 1], want["frame"] % nb)
    np.testing.assert_array_equal(got[:, 2:4], np.stack([want["range"], want["doppler"]], 1))
    np.testing.assert_array_equal(got[:, 4].astype(np.float32), want["mag"])
    np.testing.assert_array_equal(got[:, 5].astype(np.float32), want["threshold"])
    np.testing.assert_allclose(got[:, 6], nus[want["frame"] % nb], atol=5e-7)
    np.testing.assert_allclose(got[:, 7], nus[want["frame"] % nb] / 0.25, atol=5e-7)
