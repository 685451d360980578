"""Bearing estimation on the GPU (fmcw_bearings_* of libfmcw.so on gfx950 through the C-ABI), every
case against tests/bearings_ref.py (the specification in fp64 NumPy) run on the GPU's own
fmcw_range_ct output downloaded to the host.  The tolerances are bearings_ref.assert_bearings_match's
(derived there); every comparison prints the worst fraction of each bound it used.

Shapes: n_range 64 with n_doppler 32 (fewer chirps than lanes), 64 (one per lane) and 128, and
128 x 1024 (a lane takes 16 chirps and d * c reaches its largest value); n_rx 1..4; MTI off, 2- and
3-pulse; Hamming and no window; 2 frames (one of each synthetic recipe).  The full-scale cases take
records in every range row and Doppler bin of a white Gaussian spectrum (bearings_ref.full_scale_case),
not at detections.  run() also fails on any word of the records or snapshots written that still holds
the sentinel.
"""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

import fmcw_oracle as O
from fmcw import (BEARING_DTYPE, DET_DTYPE, PLOT_DTYPE, BearingEstimator, DeviceBuffer, PlotExtractor, RadarCore, cli,
                  formats, synth)
import bearings_ref as BR
from bearings_ref import assert_bearings_match, bearings_ref
from gpu_support import SENTINEL, Hip, assert_all_written

pytestmark = pytest.mark.gpu

NF = 2
MAX_LIST = 300    # detections kept per case (every k-th of the path's list): the reference is O(n n_rx n_doppler)


def two_recipe_cube(nr, nc, nrx, seed=40, rx_phase=0.25):
    return np.ascontiguousarray(np.concatenate([
        synth.frames(1, nr, nc, nrx, "two_targets", seed=seed, rx_phase=rx_phase),
        synth.frames(1, nr, nc, nrx, "random_target", seed=seed + 1, rx_phase=rx_phase)]))


def path_outputs(cube, nr, nc, nrx, mti, win):
    """The path's own 1-D CFAR detections of `cube`, and fmcw_range_ct's spectrum on the host with
    one zeroed frame appended (what an estimator that forgot its range check would read)."""
    nf = len(cube)
    with RadarCore(N_RANGE=nr, N_DOPPLER=nc, N_RX=nrx, cfar="os1d", max_frames=nf, window=win,
                   mti_bypass=mti == 0, NOTCH_MODE=mti or 2) as core:
        out = core.process(cube, want_map=False)
        dc = DeviceBuffer(cube.nbytes)
        dc.upload(cube)
        fb = nrx * nr * nc * 8
        ds = DeviceBuffer((nf + 1) * fb)
        ds.upload(np.zeros((nf + 1) * fb, np.uint8))
        core.range_ct(dc, ds, nf)
        spec = ds.download(np.complex64, (nf + 1, nrx, nr, nc))
        dc.free()
        ds.free()
    assert not np.any(spec[nf]) and np.any(spec[nf - 1])
    return out.dets, spec


@functools.lru_cache(maxsize=None)
def scene(nr, nc, nrx, mti, win):
    cube = two_recipe_cube(nr, nc, nrx)
    dets, spec = path_outputs(cube, nr, nc, nrx, mti, win)
    assert len(dets) > 8
    hand = np.zeros(7, DET_DTYPE)
    #                 d = 0, r = 0   d, r at their last   last frame      a duplicate of it   an unsorted pair
    for i, (f, r, d) in enumerate([(0, 0, 0), (0, nr - 1, nc - 1), (NF - 1, 9, 3), (NF - 1, 9, 3),
                                   (1, 5, nc - 1), (0, nr - 1, 0), (0, 7, 2)]):
        hand[i] = (f, r, d, 0.0, 0.0)
    recs = np.concatenate([dets[:: max(1, len(dets) // MAX_LIST)], hand])
    for a in (cube, dets, spec, recs):
        a.setflags(write=False)
    return SimpleNamespace(cube=cube, dets=dets, spec=spec, recs=recs, nr=nr, nc=nc, nrx=nrx, mti=mti, win=win)


def run(be, spec, n_frames, recs, rec_cap=None, n_word=None, snaps=True):
    """One fmcw_bearings_enqueue on host data.  Returns (status words, bearings written, the
    sentinel-filled bearing buffer's bytes after them, snapshots written or None, the snapshot buffer's
    bytes after them or None)."""
    n, stride = len(recs), recs.dtype.itemsize
    nrx = spec.shape[1]
    rec_cap = n if rec_cap is None else rec_cap
    bufs = []

    def dev(nbytes, fill=None):
        b = DeviceBuffer(max(nbytes, 8))
        bufs.append(b)
        if fill is not None:
            b.upload(np.full(max(nbytes, 8), fill, np.uint8))
        return b
    dspec = dev(spec.nbytes)
    dspec.upload(spec)
    drec = dev(n * stride)
    if n:
        drec.upload(recs)
    dn = dev(4)
    dn.upload(np.array([n if n_word is None else n_word, 0], np.uint32))
    slots = max(n, rec_cap) + 4
    db = dev(slots * 32, SENTINEL)
    dsn = dev(slots * nrx * 8, SENTINEL) if snaps else None
    dst = dev(8)
    dst.upload(np.array([0xDEAD, 0xBEEF], np.uint32))
    be.enqueue(dspec, n_frames, drec, stride, rec_cap, dn, db, dsn, dst)
    st = dst.download(np.uint32, (2,))
    k = int(st[0])
    assert k <= slots - 4
    raw = db.download(np.uint8, (slots * 32,))
    assert_all_written(raw[: k * 32], "bearings")
    got, rest = raw[: k * 32].view(BEARING_DTYPE).copy(), raw[k * 32:]
    sn = sn_rest = None
    if snaps:
        raw = dsn.download(np.uint8, (slots * nrx * 8,))
        assert_all_written(raw[: k * nrx * 8], "snapshots")
        sn, sn_rest = raw[: k * nrx * 8].view(np.complex64).reshape(k, nrx).copy(), raw[k * nrx * 8:]
    for b in bufs:
        b.free()
    return st, got, rest, sn, sn_rest


def estimator(sc, **kw):
    return BearingEstimator(sc.nr, sc.nc, sc.nrx, window=sc.win, mti=sc.mti, **kw)


def check(sc, recs, label, n_frames=NF, **kw):
    ref = bearings_ref(sc.spec, recs, n_frames=n_frames, win=sc.win, mti=sc.mti)
    with estimator(sc, **kw) as be:
        st, got, rest, sn, sn_rest = run(be, sc.spec, n_frames, recs)
    bad = int(np.sum(ref[0]["flags"] & 4 != 0))
    assert list(st) == [len(recs), bad], st
    used = assert_bearings_match(got, sn, *ref, label=label)
    print(f"\n{label}: {len(recs)} records, fraction of each bound used: " +
          ", ".join(f"{k} {v:.3g}" for k, v in used.items()))
    assert np.all(rest == SENTINEL) and np.all(sn_rest == SENTINEL)
    return got, sn


GEOMS = [(64, 32), (64, 64), (64, 128), (128, 1024)]


@pytest.mark.parametrize("mti", [0, 2, 3])
@pytest.mark.parametrize("nrx", [1, 2, 3, 4])
@pytest.mark.parametrize("nr,nc", GEOMS)
def test_against_reference(gpu, nr, nc, nrx, mti):
    """The path's detections of both recipes plus the hand-placed records (first and last Doppler
    bin and range row, the last frame, a duplicate, an unsorted pair); the window alternates over the
    matrix so that both meet every n_rx, MTI mode and geometry -- except Hamming with the 3-pulse
    canceller at n_doppler 1024, which test_window_and_mti_at_one_shape has at 128: two_targets sits
    at Doppler 5 / 1024 and -10 / 1024, inside that canceller's notch, where the Hamming-weighted |s_k|
    falls to 1e-4 of A_k and the reference itself (fp64, before any GPU value) finds 28 % of the
    list ill-conditioned for nu, against the 5 % a case may skip; without the window it is 2.6 %."""
    win = "none" if (nrx + mti + GEOMS.index((nr, nc))) % 2 or (nc == 1024 and mti == 3) else "hamming"
    sc = scene(nr, nc, nrx, mti, win)
    got, sn = check(sc, sc.recs, f"{nr}x{nc} rx{nrx} mti{mti} {win}")
    n = len(sc.recs)
    assert got[n - 4].tobytes() == got[n - 5].tobytes() and sn[n - 4].tobytes() == sn[n - 5].tobytes()  # the duplicate
    if nrx == 1:
        assert np.all(got["flags"] == 2)
    else:
        # both recipes place their targets a quarter cycle per element apart
        strong = got["power"] > 0.5 * got["power"].max()
        assert np.all(np.abs(got["nu"][strong] - 0.25) < 0.01) and np.all(got["coherence"][strong] > 0.99)


@pytest.mark.parametrize("mti", BR.FS_MTIS)
@pytest.mark.parametrize("nc", BR.FS_DOPPLERS)
def test_full_scale_against_reference(gpu, nc, mti):
    """Records that are no detections: 8 cells in every range row of both frames of the beamformer's
    full-scale scene (white Gaussian cells from the host), every Doppler bin among them.  Every row's
    snapshot is then at the scale of its bound, where a detection list visits the targets' rows alone:
    a wrong row, frame or channel stride, or a wrong canceller edge, is out of bound wherever it falls.
    tests/test_bearings_host.py: the reference alone leaves at most 12 of the 1024 records to the 5 % a
    case may skip for nu."""
    spec, recs, win = BR.full_scale_case(nc, mti)
    assert recs.dtype == DET_DTYPE
    sc = SimpleNamespace(spec=spec, nr=BR.FS_NR, nc=nc, nrx=BR.FS_NRX, mti=mti, win=win)
    got, sn = check(sc, recs, f"full scale {BR.FS_NR}x{nc} rx{BR.FS_NRX} mti{mti} {win}", n_frames=BR.FS_NF)
    assert not np.any(got["flags"] & 6)


@pytest.mark.parametrize("win", ["hamming", "none"])
@pytest.mark.parametrize("mti", [0, 2, 3])
def test_window_and_mti_at_one_shape(gpu, win, mti):
    """Every window x MTI pair at one shape (the matrix above alternates the window)."""
    sc = scene(64, 128, 4, mti, win)
    check(sc, sc.recs, f"64x128 rx4 mti{mti} {win}")


def test_other_bearings(gpu):
    """Targets at rx_phase 0.125 and -0.25 (64 x 32 x 4 rx): the reference comparison away from a
    quarter cycle, and end to end the records at the two peak cells give those nu within 0.01 --
    through estimate() on a host spectrum, with DET_DTYPE and PLOT_DTYPE records."""
    nr, nc, nrx = 64, 32, 4
    cube = np.ascontiguousarray(synth.frames(NF, nr, nc, nrx, "two_targets", seed=50, rx_phase=[0.125, -0.25]))
    dets, spec = path_outputs(cube, nr, nc, nrx, 0, "hamming")
    sc = SimpleNamespace(spec=spec, nr=nr, nc=nc, nrx=nrx, mti=0, win="hamming")
    got, _ = check(sc, dets, "rx_phase 0.125 / -0.25")
    peaks = {(100 * nr // 1024, 5): 0.125, (500 * nr // 1024, nc - 10): -0.25}
    cells = list(zip(got["range"].tolist(), got["doppler"].tolist()))
    for cell, nu in peaks.items():
        hit = [i for i, c in enumerate(cells) if c == cell]
        assert len(hit) == NF, (cell, hit)            # the path detects the peak cell in both frames
        assert np.all(np.abs(got["nu"][hit] - nu) < 0.01), (cell, got["nu"][hit])
        assert np.all(got["coherence"][hit] > 0.99)
    with BearingEstimator(nr, nc, nrx, max_records=len(dets)) as be:
        b16, s16 = be.estimate(spec[:NF], dets)
        plots = np.zeros(len(dets), PLOT_DTYPE)
        for k in ("frame", "range", "doppler", "mag"):
            plots[k] = dets[k]
        b32, s32 = be.estimate(spec[:NF], plots)
        assert b16.tobytes() == got.tobytes() == b32.tobytes() and s16.tobytes() == s32.tobytes()
        assert be.estimate(spec[:NF], dets, want_snaps=False)[1] is None
        with pytest.raises(TypeError):
            be.estimate(spec[:NF], np.zeros(3, np.float32))
    # spacing 0.2 wavelengths: nu = -0.25 has no real angle (flag 1), nu = 0.125 has
    rec = np.zeros(2, DET_DTYPE)
    rec["range"], rec["doppler"] = [c[0] for c in peaks], [c[1] for c in peaks]
    ref = bearings_ref(spec, rec, n_frames=NF, spacing=0.2)
    with BearingEstimator(nr, nc, nrx, spacing=0.2) as be:
        st, g, _, sn, _ = run(be, spec, NF, rec)
    assert_bearings_match(g, sn, *ref, spacing=0.2, label="spacing 0.2")
    assert list(g["flags"]) == [0, 1] and abs(g["sin_theta"][1] + 1.25) < 0.05


@pytest.mark.parametrize("mti", [0, 2, 3])
@pytest.mark.parametrize("nr,nc,nrx", [(64, 32, 4), (64, 128, 2)])
def test_power_is_the_path_magnitude(gpu, nr, nc, nrx, mti):
    """power against the mag of the same fmcw_process detections (Hamming, the same MTI, |X| NCI,
    linear map, fp32 spectrum): within 2e-4 of the oracle's frame peak -- the suite's 1e-4 per frame
    for the map, once for each side."""
    sc = scene(nr, nc, nrx, mti, "hamming")
    with estimator(sc, max_records=len(sc.dets)) as be:
        got, _ = be.estimate(sc.spec[:NF], sc.dets, want_snaps=False)
    worst = 0.0
    for f in range(NF):
        peak = O.process(sc.cube[f], None, mti_mode=mti)["mag"].max()
        m = sc.dets["frame"] == f
        assert m.any()
        worst = max(worst, float(np.abs(got["power"][m].astype(np.float64) - sc.dets["mag"][m]).max() / peak))
    print(f"\n{nr}x{nc} rx{nrx} mti{mti}: max |power - mag| = {worst:.3g} of the frame peak (bound 2e-4)")
    assert worst <= 2e-4


def test_stride_32_on_plots(gpu):
    """The plot extractor's output of the path's list as the record list (stride 32): the reference,
    and the same bytes as stride 16 on the same cells."""
    sc = scene(64, 128, 4, 0, "hamming")
    with PlotExtractor(sc.nr, sc.nc, max_dets=len(sc.dets)) as px:
        plots = px.extract(sc.dets)
    assert 2 <= len(plots) < len(sc.dets)
    got, sn = check(sc, plots, "plots, stride 32")
    as_dets = np.zeros(len(plots), DET_DTYPE)
    for k in ("frame", "range", "doppler"):
        as_dets[k] = plots[k]
    got16, sn16 = check(sc, as_dets, "the plots' cells, stride 16")
    assert got.tobytes() == got16.tobytes() and sn.tobytes() == sn16.tobytes()


def test_bad_stride_is_einval(gpu):
    sc = scene(64, 32, 2, 0, "hamming")
    from fmcw import FmcwError
    with estimator(sc) as be:
        d = DeviceBuffer(64)
        for stride in (0, 8, 24, 48):
            with pytest.raises(FmcwError, match="rec_stride"):
                be.enqueue(d, NF, d, stride, 1, d, d, None, d)
        d.free()


def test_counts_and_untouched_bytes(gpu):
    """A count word of 0; above rec_cap; above max_records; a count that is no multiple of the 4
    records a workgroup has in flight; snaps_dev NULL.  Bytes beyond the n records stay as they were."""
    sc = scene(64, 64, 3, 2, "hamming")
    recs = sc.recs[:23]
    ref = bearings_ref(sc.spec, recs, n_frames=NF, win=sc.win, mti=sc.mti)
    with estimator(sc) as be:
        st, got, rest, sn, sn_rest = run(be, sc.spec, NF, recs, n_word=0)
        assert list(st) == [0, 0] and len(got) == 0 and np.all(rest == SENTINEL) and np.all(sn_rest == SENTINEL)
        st, got, rest, sn, sn_rest = run(be, sc.spec, NF, recs[:0], rec_cap=0, n_word=5)      # no record kernel at all
        assert list(st) == [0, 0] and np.all(rest == SENTINEL)
        full = run(be, sc.spec, NF, recs)
        assert list(full[0]) == [23, 0]
        assert_bearings_match(full[1], full[3], *ref)
        for n_word, cap in ((40, 17), (23, 21), (0xFFFFFFFF, 22)):                             # rec_cap binds
            st, got, rest, sn, sn_rest = run(be, sc.spec, NF, recs, rec_cap=cap, n_word=n_word)
            assert list(st) == [cap, 0]
            assert got.tobytes() == full[1][:cap].tobytes() and sn.tobytes() == full[3][:cap].tobytes()
            assert np.all(rest == SENTINEL) and np.all(sn_rest == SENTINEL)
        st, got, rest, sn, _ = run(be, sc.spec, NF, recs, snaps=False)
        assert sn is None and list(st) == [23, 0] and got.tobytes() == full[1].tobytes() and np.all(rest == SENTINEL)
    with estimator(sc, max_records=10) as be:                                                  # max_records binds
        st, got, rest, sn, sn_rest = run(be, sc.spec, NF, recs)
        assert list(st) == [10, 0] and got.tobytes() == full[1][:10].tobytes()
        assert np.all(rest == SENTINEL) and np.all(sn_rest == SENTINEL)


def test_out_of_range_records(gpu):
    """One record per kind (frame = n_frames, range = n_range, doppler = n_doppler) among good ones.
    The spectrum buffer holds one zeroed frame more than n_frames, so an estimator without the check
    reads defined memory and fails by value: flag 4, zeros, status word 1 = 3."""
    for nrx, mti in ((4, 0), (1, 3)):
        sc = scene(64, 32, nrx, mti, "hamming")
        recs = sc.recs[:9].copy()
        recs["frame"][1] = NF
        recs["range"][4] = sc.nr
        recs["doppler"][6] = sc.nc
        ref = bearings_ref(sc.spec, recs, n_frames=NF, win=sc.win, mti=sc.mti)
        with estimator(sc) as be:
            st, got, rest, sn, sn_rest = run(be, sc.spec, NF, recs)
        assert list(st) == [9, 3]
        assert_bearings_match(got, sn, *ref)
        for i in (1, 4, 6):
            assert got[i].tobytes() == np.array([(0, 0, 0, 4, 0, 0, 0, 0, 0)], BEARING_DTYPE).tobytes()
            assert not np.any(sn[i])
        assert np.all(got["flags"][[0, 2, 3, 5, 7, 8]] & 4 == 0) and np.all(got["power"][[0, 2, 3, 5, 7, 8]] > 0)
        assert np.all(rest == SENTINEL) and np.all(sn_rest == SENTINEL)
        # a call with n_frames = 1 puts every record of frame 1 out of range
        with estimator(sc) as be:
            st, got, _, _, _ = run(be, sc.spec, 1, sc.recs)
        assert st[1] == np.sum(sc.recs["frame"] >= 1) > 0 and np.all((got["flags"] & 4 != 0) == (sc.recs["frame"] >= 1))


@pytest.mark.parametrize("nr,nc,nrx,mti", [(64, 32, 4, 0), (128, 1024, 2, 2)])
def test_capped_grid(gpu, nr, nc, nrx, mti):
    """1 and 3 workgroups through the hook (a wave takes every 4th / 12th record; 3 x 4 does not
    divide the count), then the built-in grid again, on the same object: the reference's values, and
    the same bytes each time."""
    sc = scene(nr, nc, nrx, mti, "hamming")
    recs = sc.recs[: len(sc.recs) - (len(sc.recs) % 12 == 0)]
    assert len(recs) > 40 and len(recs) % 12
    ref = bearings_ref(sc.spec, recs, n_frames=NF, win=sc.win, mti=sc.mti)
    with estimator(sc) as be:
        st0, got0, rest0, sn0, snr0 = run(be, sc.spec, NF, recs)
        assert_bearings_match(got0, sn0, *ref)
        for grid in (1, 3, 0):
            be.set_grid_for_test(grid)
            st, got, rest, sn, snr = run(be, sc.spec, NF, recs)
            assert list(st) == list(st0) == [len(recs), 0], grid
            assert got.tobytes() == got0.tobytes() and sn.tobytes() == sn0.tobytes(), grid
            assert np.all(rest == SENTINEL) and np.all(snr == SENTINEL)


def test_graph_replay_on_a_second_list(gpu):
    """fmcw_bearings_enqueue captured into a graph, replayed on two lists of different lengths (the
    count is read on the device) and on the first again."""
    sc = scene(64, 64, 4, 0, "hamming")
    lists = [sc.recs[:37], sc.recs[37:90][::-1].copy()]
    assert len(lists[1]) == 53
    cap = 64
    hip = Hip()
    with estimator(sc) as be:
        dspec = DeviceBuffer(sc.spec.nbytes)
        dspec.upload(sc.spec)
        drec, dn = DeviceBuffer(cap * 16), DeviceBuffer(4)
        db, dsn, dst = DeviceBuffer(cap * 32), DeviceBuffer(cap * sc.nrx * 8), DeviceBuffer(8)
        try:
            with hip.graph(lambda s: be.enqueue(dspec, NF, drec, 16, cap, dn, db, dsn, dst, stream=s.value)) as (exe, s):
                seen = []
                for k in (0, 1, 0):
                    recs = lists[k]
                    drec.upload(recs)
                    dn.upload(np.array([len(recs)], np.uint32))
                    hip.replay(exe, s)
                    assert list(dst.download(np.uint32, (2,))) == [len(recs), 0]
                    got = db.download(BEARING_DTYPE, (len(recs),))
                    sn = dsn.download(np.complex64, (len(recs), sc.nrx))
                    assert_bearings_match(got, sn, *bearings_ref(sc.spec, recs, n_frames=NF), label=f"replay {k}")
                    seen.append(got.tobytes())
                assert seen[0] == seen[2] and seen[0] != seen[1]
        finally:
            for b in (dspec, drec, dn, db, dsn, dst):
                b.free()


def test_cli_bearings(gpu, tmp_path):
    """--bearings on a 4-channel .npy writes ADR_bearings.txt: the reference on the run's own
    detections, and on its plots with --plots; the detection file is the one written without it."""
    nr, nc, nrx = 64, 32, 4
    cube = np.ascontiguousarray(synth.frames(NF, nr, nc, nrx, "two_targets", seed=50, rx_phase=[0.125, -0.25]))
    np.save(tmp_path / "cube.npy", cube)
    common = [str(tmp_path / "cube.npy"), "--n-range", str(nr), "--n-doppler", str(nc), "--cfar", "os1d"]
    cli.main(common + ["--out-dir", str(tmp_path / "plain")])
    cli.main(common + ["--out-dir", str(tmp_path / "b"), "--bearings"])
    cli.main(common + ["--out-dir", str(tmp_path / "p"), "--bearings", "--plots", "--rx-spacing", "0.25"])
    assert sorted(p.name for p in (tmp_path / "plain").iterdir()) == ["ADR_detections.txt"]
    assert sorted(p.name for p in (tmp_path / "b").iterdir()) == ["ADR_bearings.txt", "ADR_detections.txt"]
    assert (tmp_path / "b" / "ADR_detections.txt").read_bytes() == (tmp_path / "plain" / "ADR_detections.txt").read_bytes()
    dets, spec = path_outputs(cube, nr, nc, nrx, 0, "hamming")
    with PlotExtractor(nr, nc, max_dets=len(dets)) as px:
        plots = px.extract(dets)
    for name, recs, spacing in (("b", dets, 0.5), ("p", plots, 0.25)):
        want = bearings_ref(spec, recs, n_frames=NF, spacing=spacing)[0]
        got = formats.read_bearings(tmp_path / name / "ADR_bearings.txt")
        assert len(got) == len(want) > 0
        np.testing.assert_array_equal(got[:, :3], np.stack([want["frame"], want["range"], want["doppler"]], 1))
        np.testing.assert_allclose(got[:, 3], want["power"], rtol=1e-4)
        strong = want["power"] > 0.5 * want["power"].max()
        np.testing.assert_allclose(got[strong, 4], want["nu"][strong], atol=1e-4)
        np.testing.assert_allclose(got[strong, 5], want["sin_theta"][strong], atol=1e-4 / spacing)
