"""Adaptive beam weights on the GPU (fmcw_adapt_* and fmcw_beams_set_weights_dev of libfmcw.so on gfx950
through the C-ABI), every case against tests/adapt_ref.py (the specification in fp64 NumPy) on the
same uploaded spectrum, with sentinel bytes behind every output.  The bounds are adapt_ref's (derived
from the kernel's add chains); every comparison prints the worst fraction of each.

Shapes (adapt_ref): n_range 64; n_doppler 32 and 1024; n_rx 1, 2, 3, 4, 5, 8, 9, 15, 16 (8 | 9 is the
boundary between the 16-row and the 32-row accumulator tile); 1 and 3 frames; the whole map, one row
and three rows as training windows (2 and 6 units at n_doppler 32: no multiple of the 4 waves of a
workgroup); MTI off, 2- and 3-pulse; 1, 3 and 64 beams.  The full-scale cases run on the beamformer's
white Gaussian scene (adapt_ref.full_scale_case), where every unit of the accumulation weighs the same.
enqueue_checked also fails on any word of W or cov that still holds the sentinel.
"""
import functools

import numpy as np
import pytest

import fmcw_oracle as O
import adapt_ref as AR
from adapt_ref import adapt_ref, assert_matches, gamma
from beams_ref import assert_maps_match, beams_ref
from fmcw import (ADAPT_FALLBACK, DET_DTYPE, AdaptiveWeights, BeamFormer, DeviceBuffer, RadarCore, cli, formats,
                  steering_vectors, steering_weights)
from fmcw import _lib as L
from fmcw.adapt import INFO_WORDS, parse_info
from gpu_support import SENTINEL, Hip, assert_all_written, assert_sentinel_after, range_ct_spectrum, run_beams, sentinel_buffer

pytestmark = pytest.mark.gpu

TAIL = 256        # sentinel bytes kept after each output
NR = AR.NR


@functools.lru_cache(maxsize=4)
def scene(nd, nrx):
    return AR.noise_scene(nd, nrx)


def enqueue_checked(ad, dspec, n_frames, want_cov=True):
    """One fmcw_adapt_enqueue on a device spectrum into sentinel-filled buffers: (W, R, info, raw bytes
    of the three outputs), after checking that the bytes behind every output kept the sentinel."""
    c = ad.cfg
    sizes = (ad.w_bytes(), ad.cov_bytes(), 4 * INFO_WORDS)
    bufs = [sentinel_buffer(n + TAIL) for n in sizes]
    ad.enqueue(dspec, n_frames, bufs[0], bufs[1] if want_cov else None, bufs[2])
    raws = [b.download(np.uint8, (n + TAIL,)) for b, n in zip(bufs, sizes)]
    for b in bufs:
        b.free()
    for raw, n, name in zip(raws, sizes, ("w", "cov", "info")):
        assert_sentinel_after(raw, n, 1, name)
    if not want_cov:
        assert np.all(raws[1] == SENTINEL), "cov_dev is NULL but cov was written"
    else:
        assert_all_written(raws[1][:sizes[1]], "cov")
    assert_all_written(raws[0][:sizes[0]], "w")
    W = raws[0][:sizes[0]].view(np.complex64).reshape(c.n_beams, c.n_rx).copy()
    R = raws[1][:sizes[1]].view(np.complex128).reshape(c.n_rx, c.n_rx).copy()
    words = raws[2][:sizes[2]].view(np.uint32).copy()
    assert words[6] == 0 and words[7] == 0
    return W, R, parse_info(words), b"".join(r[:n].tobytes() for r, n in zip(raws, sizes))


def run(ad, spec, n_frames=None, want_cov=True):
    dspec = DeviceBuffer(max(spec.nbytes, 8))
    dspec.upload(spec)
    try:
        return enqueue_checked(ad, dspec, len(spec) if n_frames is None else n_frames, want_cov)
    finally:
        dspec.free()


def check(spec, a, loading, mti, r0, rows, label, dspec=None):
    nf, nrx, nr, nd = spec.shape
    ref = adapt_ref(spec, a, float(np.float32(loading)), mti, r0, rows)
    with AdaptiveWeights(nr, nd, nrx, a, loading=loading, mti=mti, train_r0=r0, train_rows=rows) as ad:
        W, R, info, _ = run(ad, spec) if dspec is None else enqueue_checked(ad, dspec, nf)
    assert info["n_units"] == AR.chain_length(nf, rows, nd)[1]
    assert_matches(W, R, info, ref, gamma(nf, rows, nd), loading, label)
    gain = np.einsum("bk,bk->b", W.astype(np.complex128), np.asarray(a).astype(np.complex128))
    assert np.allclose(gain, 1.0, atol=1e-5), f"{label}: W a = {gain}"
    return W, R, info


@pytest.mark.parametrize("mti", AR.MTIS)
@pytest.mark.parametrize("nrx", AR.RXS)
@pytest.mark.parametrize("nd", AR.DOPPLERS)
def test_against_reference(gpu, nd, nrx, mti):
    """Steering vectors and one random complex constraint matrix per case, 3 beams; the frame count
    and the training window alternate over the matrix (adapt_ref.matrix_case)."""
    nf, (r0, rows, loading) = AR.matrix_case(nd, nrx, mti)
    spec = scene(nd, nrx)[:nf]
    dspec = DeviceBuffer(spec.nbytes)
    dspec.upload(spec)
    try:
        for name, a in zip(("steering", "random"), AR.case_constraints(nrx, 3, seed=1000 * nd + 10 * nrx + mti)):
            check(spec, a, loading, mti, r0, rows,
                  f"{NR}x{nd} rx{nrx} mti{mti} frames{nf} rows[{r0},{r0 + rows}) {name}", dspec)
    finally:
        dspec.free()


@pytest.mark.parametrize("mti", AR.MTIS)
@pytest.mark.parametrize("nrx", AR.FS_RXS)
@pytest.mark.parametrize("nd", AR.DOPPLERS)
def test_full_scale_against_reference(gpu, nd, nrx, mti):
    """The beamformer's full-scale scene (white Gaussian cells, 2 frames, the whole map as the training
    window): every row, frame and chirp weighs the same in R, so a unit left out, taken twice or
    cancelled against the wrong predecessor moves cov by about 1 / n_units of its scale, against a bound
    of gamma.  tests/test_adapt_host.py: the reference takes no fallback here."""
    spec, a = AR.full_scale_case(nd, nrx, mti)
    check(spec, a, AR.FS_LOADING, mti, 0, NR, f"full scale {NR}x{nd} rx{nrx} mti{mti} frames{AR.FS_NF}")


@pytest.mark.parametrize("mti", AR.MTIS)
@pytest.mark.parametrize("nf", AR.FRAMES)
@pytest.mark.parametrize("window", AR.WINDOWS)
@pytest.mark.parametrize("nrx", [4, 16])
def test_windows_frames_and_mti_at_one_shape(gpu, nrx, window, nf, mti):
    """Every training window x frame count x MTI mode at n_doppler 32 with both accumulator tiles
    (the matrix above alternates them).  The three-row window gives 2 and 6 units."""
    r0, rows, loading = window
    a = AR.case_constraints(nrx, 3, seed=nrx + nf)[1]
    check(scene(32, nrx)[:nf], a, loading, mti, r0, rows, f"{NR}x32 rx{nrx} mti{mti} frames{nf} rows[{r0},{r0 + rows})")


@pytest.mark.parametrize("nf", AR.FRAMES)
@pytest.mark.parametrize("nrx", [8, 9])
def test_training_run_shorter_than_a_step(gpu, nrx, nf):
    """One training row at n_doppler 32 under the 3-pulse canceller, at the last n_rx of the 16-row tile
    and the first of the 32-row one.  A frame's run is half a 64-point step: lanes 32 .. 63 fall back to
    point 0 as chirp 0, where the canceller's predecessor loads are clamped, and must add nothing.  The
    row is not the map's first, so what lies before its chirp 0 in memory is the previous row's last
    chirps, which the zero delay line drops."""
    r0, rows, loading = AR.WINDOWS[1]
    assert rows * 32 < 64 and r0 > 0
    a = AR.case_constraints(nrx, 3, seed=nrx + nf)[1]
    check(scene(32, nrx)[:nf], a, loading, 3, r0, rows, f"{NR}x32 rx{nrx} mti3 frames{nf} rows[{r0},{r0 + rows})")


@pytest.mark.parametrize("nb", [1, 3, 64])
def test_beam_counts(gpu, nb):
    for nrx in (5, 16):
        a = AR.case_constraints(nrx, nb, seed=nb)[0]
        W, _, _ = check(scene(32, nrx), a, 1e-3, 0, 0, NR, f"{NR}x32 rx{nrx} beams{nb}")
        assert W.shape == (nb, nrx)


@pytest.mark.parametrize("nd,nrx,mti,window", [(32, 3, 0, 2), (1024, 16, 2, 0), (32, 9, 3, 0), (1024, 4, 0, 2)])
def test_grid_independence(gpu, nd, nrx, mti, window):
    """1 and 3 workgroups through the hook, then the built-in grid again, on the same object and 3
    frames: a wave then passes several units (at 1024 x 64 rows, 2048 units over 4 waves).  W, cov and
    info are the same bytes each time."""
    r0, rows, loading = AR.WINDOWS[window]
    spec = scene(nd, nrx)
    a = AR.case_constraints(nrx, 3, seed=nd + nrx)[1]
    ref = adapt_ref(spec, a, float(np.float32(loading)), mti, r0, rows)
    with AdaptiveWeights(NR, nd, nrx, a, loading=loading, mti=mti, train_r0=r0, train_rows=rows) as ad:
        W, R, info, base = run(ad, spec)
        assert_matches(W, R, info, ref, gamma(3, rows, nd), loading, f"{NR}x{nd} rx{nrx} mti{mti} built-in grid")
        for grid in (1, 3, 0):
            ad.set_grid_for_test(grid)
            assert run(ad, spec)[3] == base, grid


def test_info_and_fallback_on_a_rank_deficient_input(gpu):
    """n_rx 4 with channel 2 a copy of channel 1 and no loading: R is singular, the call writes the
    conventional weights and sets FMCW_ADAPT_FALLBACK; cov, K and delta are written as ever.  With
    loading the same input solves."""
    spec = np.array(scene(32, 4)[:1])
    spec[:, 2] = spec[:, 1]
    a = AR.case_constraints(4, 3, seed=5)[1]
    ref = adapt_ref(spec, a, 0.0)
    assert ref["flags"] == AR.FALLBACK
    with AdaptiveWeights(NR, 32, 4, a, loading=0.0) as ad:
        W, R, info, _ = run(ad, spec)
    assert info["fallback"] and info["flags"] == ADAPT_FALLBACK == AR.FALLBACK
    assert info["K"] == NR * 32 and info["delta"] == 0.0
    assert np.abs(R - ref["R"]).max() <= gamma(1, NR, 32) * ref["A"].max()
    np.testing.assert_allclose(W, AR.conventional(a), rtol=2.0 ** -22, atol=0)
    check(spec, a, 1e-2, 0, 0, NR, "rank-deficient input with loading")



def test_null_cov_and_zero_frames(gpu):
    """cov_dev NULL: W and info are the bytes of the call with it, cov untouched.  n_frames == 0 looks
    at nothing and writes nothing; bad pointers are FMCW_EINVAL and write nothing."""
    lib = L.load()
    spec = scene(32, 5)
    a = AR.case_constraints(5, 3, seed=2)[0]
    with AdaptiveWeights(NR, 32, 5, a, loading=1e-3) as ad:
        W, _, info, _ = run(ad, spec)
        W2, _, info2, _ = run(ad, spec, want_cov=False)
        assert W.tobytes() == W2.tobytes() and info == info2
        d = sentinel_buffer(2 * TAIL)
        ad.enqueue(d, 0, d, d, d)
        assert lib.fmcw_adapt_enqueue(ad._h, None, 0, None, None, None, None) == L.FMCW_OK
        assert lib.fmcw_adapt_enqueue(ad._h, None, 1, d.ptr, None, d.ptr, None) == L.FMCW_EINVAL
        assert lib.fmcw_adapt_enqueue(ad._h, d.ptr, 1, d.ptr, d.ptr + 8, d.ptr, None) == L.FMCW_EINVAL
        assert b"16-byte" in lib.fmcw_last_error()
        assert np.all(d.download(np.uint8, (2 * TAIL,)) == SENTINEL)
        d.free()


# ---- the chain on the jammer scene -----------------------------------------------------------------
def os2d_cells(dets):
    return set(zip(dets["range"].tolist(), dets["doppler"].tolist()))


def test_chain_on_the_jammer_scene(gpu):
    """enqueue -> fmcw_beams_set_weights_dev -> fmcw_beams_enqueue -> fmcw_cfar (2-D OS-CFAR) on
    adapt_ref.jammer_scene, outputs on the device only: the target cell is detected with the adaptive
    weights and missed with the conventional ones of the same beamformer before the update; both maps
    within beams_ref's tolerance of the reference maps (the adaptive one formed with W_ref)."""
    nr, nc, nrx = AR.JAM_NR, AR.JAM_NC, AR.JAM_NRX
    spec = AR.jammer_scene()
    a = steering_vectors(nrx, [AR.JAM_NU_T])
    wc = steering_weights(nrx, [AR.JAM_NU_T])
    ref = adapt_ref(spec, a, 1e-2)
    with AdaptiveWeights(nr, nc, nrx, a, loading=1e-2) as ad, BeamFormer(nr, nc, nrx, wc) as bf, \
            RadarCore(N_RANGE=nr, N_DOPPLER=nc, N_RX=1, cfar="os2d", max_frames=1) as core:
        dspec = DeviceBuffer(spec.nbytes)
        dspec.upload(spec)
        dw, di, dm = DeviceBuffer(ad.w_bytes()), DeviceBuffer(4 * INFO_WORDS), DeviceBuffer(bf.maps_frame_bytes())
        cap = nr * nc
        dd, dn = DeviceBuffer(cap * 16), DeviceBuffer(16)
        got = {}
        for kind in ("conventional", "adaptive"):
            if kind == "adaptive":
                ad.enqueue(dspec, 1, dw, None, di)
                bf.set_weights_dev(dw)
            bf.enqueue(dspec, 1, dm)
            core.cfar(dm, 1, dd, cap, dn)
            st = dn.download(np.uint32, (4,))
            assert st[1] == 0 and st[0] <= cap
            got[kind] = (dm.download(np.float32, (1, 1, nr, nc)), dd.download(DET_DTYPE, (int(st[0]),)))
        W = dw.download(np.complex64, (1, nrx))
        info = parse_info(di.download(np.uint32, (INFO_WORDS,)))
        for b in (dspec, dw, di, dm, dd, dn):
            b.free()
    assert not info["fallback"] and info["K"] == nr * nc
    assert_maps_match(got["conventional"][0], *beams_ref(spec, wc), label="conventional map")
    assert_maps_match(got["adaptive"][0], *beams_ref(spec, ref["W"]), label="adaptive map (W_ref)")
    assert AR.JAM_CELL not in os2d_cells(got["conventional"][1])
    assert AR.JAM_CELL in os2d_cells(got["adaptive"][1])
    for kind, (m, dets) in got.items():    # the lists are the oracle's CFAR on the GPU's own maps
        det, thr = O.cfar_os2d(m[0, 0], O.Cfar2D())
        assert os2d_cells(dets) == set(zip(*(x.tolist() for x in np.nonzero(det)))), kind
    aj = steering_vectors(nrx, [AR.JAM_NU_J])[0].astype(np.complex128)
    null_db = 20 * np.log10(abs(W[0].astype(np.complex128) @ aj) / abs(wc[0].astype(np.complex128) @ aj))
    print(f"\nresponse at the jammer, adaptive over conventional: {null_db:.1f} dB")
    assert null_db <= -30.0


def test_chain_captured_and_replayed_on_a_second_scene(gpu):
    """The same chain captured into one graph (default queue count) and replayed on the jammer scene
    and on one with the jammer at nu = 0.42 (a sidelobe peak of the conventional beam): each replay's weights are that scene's own (within the
    reference's bound, and a null at that scene's jammer), and the target is detected both times."""
    nr, nc, nrx = AR.JAM_NR, AR.JAM_NC, AR.JAM_NRX
    scenes = [(AR.JAM_NU_J, AR.jammer_scene()), (0.42, AR.jammer_scene(seed=8, nu_j=0.42))]
    a = steering_vectors(nrx, [AR.JAM_NU_T])
    wc = steering_weights(nrx, [AR.JAM_NU_T])
    hip = Hip()
    with AdaptiveWeights(nr, nc, nrx, a, loading=1e-2) as ad, BeamFormer(nr, nc, nrx, wc) as bf, \
            RadarCore(N_RANGE=nr, N_DOPPLER=nc, N_RX=1, cfar="os2d", max_frames=1) as core:
        dspec = DeviceBuffer(scenes[0][1].nbytes)
        dw, dr, di = DeviceBuffer(ad.w_bytes()), DeviceBuffer(ad.cov_bytes()), DeviceBuffer(4 * INFO_WORDS)
        dm = DeviceBuffer(bf.maps_frame_bytes())
        cap = nr * nc
        dd, dn = DeviceBuffer(cap * 16), DeviceBuffer(16)

        def calls(s):
            ad.enqueue(dspec, 1, dw, dr, di, stream=s.value)
            bf.set_weights_dev(dw, stream=s.value)
            bf.enqueue(dspec, 1, dm, stream=s.value)
            core.cfar(dm, 1, dd, cap, dn, stream=s.value)
        try:
            with hip.graph(calls) as (exe, s):
                seen = []
                for nu_j, spec in scenes:
                    dspec.upload(spec)
                    hip.replay(exe, s)
                    W = dw.download(np.complex64, (1, nrx))
                    R = dr.download(np.complex128, (nrx, nrx))
                    info = parse_info(di.download(np.uint32, (INFO_WORDS,)))
                    ref = adapt_ref(spec, a, float(np.float32(1e-2)))
                    assert_matches(W, R, info, ref, gamma(1, nr, nc), 1e-2, f"replay, jammer at {nu_j}")
                    maps = dm.download(np.float32, (1, 1, nr, nc))
                    assert_maps_match(maps, *beams_ref(spec, ref["W"]), label=f"replay map, jammer at {nu_j}")
                    n = int(dn.download(np.uint32, (4,))[0])
                    assert AR.JAM_CELL in os2d_cells(dd.download(DET_DTYPE, (n,)))
                    aj = steering_vectors(nrx, [nu_j])[0].astype(np.complex128)
                    assert abs(W[0].astype(np.complex128) @ aj) <= 10 ** -1.5 * abs(wc[0].astype(np.complex128) @ aj)
                    seen.append(W.tobytes())
                assert seen[0] != seen[1]
        finally:
            for b in (dspec, dw, dr, di, dm, dd, dn):
                b.free()


def test_a_beamformer_that_never_updates_is_unchanged(gpu):
    """A BeamFormer that never calls set_weights_dev forms its create weights' maps (beams_ref's
    check); one that was updated forms them again, byte for byte, after its own weights are set back."""
    nrx, nc = 4, 64
    spec = np.ascontiguousarray(AR.noise_scene(nc, nrx)[:2])
    w = steering_weights(nrx, [0.1, -0.25, 0.4])
    other = AR.case_constraints(nrx, 3, seed=9)[1]
    with BeamFormer(NR, nc, nrx, w) as plain, BeamFormer(NR, nc, nrx, w) as bf:
        base = run_beams(plain, spec)
        assert_maps_match(base, *beams_ref(spec, w), label="never updated")
        assert run_beams(bf, spec).tobytes() == base.tobytes()
        dw = DeviceBuffer(other.nbytes)
        dw.upload(other)
        bf.set_weights_dev(dw)
        assert_maps_match(run_beams(bf, spec), *beams_ref(spec, other), label="updated")
        dw.upload(w)
        bf.set_weights_dev(dw)
        assert run_beams(bf, spec).tobytes() == base.tobytes()
        assert run_beams(plain, spec).tobytes() == base.tobytes()
        dw.free()


def test_solve_and_cli(gpu, tmp_path):
    """solve() on a host spectrum and on a device one gives enqueue's values; --adaptive on a small
    4-channel cube writes the beam detections of the chain run by hand (range_ct -> adapt ->
    set_weights_dev -> beams -> cfar) and leaves the plain detection file as it is without it."""
    from fmcw import synth
    nc, nrx, nb = 64, 4, 4
    cube = np.ascontiguousarray(synth.frames(2, NR, nc, nrx, "two_targets", seed=40, rx_phase=[0.25, -0.125]))
    spec = range_ct_spectrum(cube, NR, nc, nrx)
    nus = (np.arange(nb) - nb // 2) / nb
    with AdaptiveWeights(NR, nc, nrx, steering_vectors(nrx, nus), loading=0.05) as ad, \
            BeamFormer(NR, nc, nrx, steering_weights(nrx, nus)) as bf:
        W, R, info, _ = run(ad, spec)
        W2, R2, info2 = ad.solve(spec)
        assert W.tobytes() == W2.tobytes() and R.tobytes() == R2.tobytes() and info == info2
        ds = DeviceBuffer(spec.nbytes)
        ds.upload(spec)
        assert ad.solve(ds)[0].tobytes() == W.tobytes()
        dw = DeviceBuffer(W.nbytes)
        dw.upload(W)
        bf.set_weights_dev(dw)
        maps = run_beams(bf, spec)
        ds.free()
        dw.free()
    np.save(tmp_path / "cube.npy", cube)
    common = [str(tmp_path / "cube.npy"), "--n-range", str(NR), "--n-doppler", str(nc), "--cfar", "os1d"]
    cli.main(common + ["--out-dir", str(tmp_path / "b"), "--beams", str(nb), "--rx-spacing", "0.25"])
    cli.main(common + ["--out-dir", str(tmp_path / "a"), "--beams", str(nb), "--rx-spacing", "0.25",
                       "--adaptive", "0.05"])
    assert (tmp_path / "a" / "ADR_detections.txt").read_bytes() == (tmp_path / "b" / "ADR_detections.txt").read_bytes()
    want = []
    for m, mp in enumerate(maps.reshape(2 * nb, NR, nc)):
        det, thr = O.cfar_os1d(mp, O.Cfar1D())
        want.append(O.detections(det, mp, thr, frame=m))
    want = np.concatenate(want)
    got = formats.read_beam_detections(tmp_path / "a" / "ADR_beam_detections.txt")
    assert len(got) == len(want) > 0
    np.testing.assert_array_equal(got[:, 0], want["frame"] // nb)
    np.testing.assert_array_equal(got[:, 1], want["frame"] % nb)
    np.testing.assert_array_equal(got[:, 2:4], np.stack([want["range"], want["doppler"]], 1))
    np.testing.assert_array_equal(got[:, 4].astype(np.float32), want["mag"])
