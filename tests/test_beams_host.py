"""The beamformer without a GPU: the C-ABI's layout, exports and argument checks (they come before any
device access), steering_weights, the specification (tests/beams_ref.py) against closed forms and the
oracle's map, the text format and the CLI's arguments."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import fmcw_oracle as O
from fmcw import _lib as L
from fmcw import DET_DTYPE, BeamFormer, cli, formats, steering_weights, synth  # noqa: F401
import beams_ref as R

NEW_SYMBOLS = ("fmcw_beams_config_default", "fmcw_beams_create", "fmcw_beams_destroy", "fmcw_beams_enqueue",
               "fmcw_beams_set_grid_for_test")


def default_cfg(lib):
    cfg = L.FmcwBeamsConfig()
    lib.fmcw_beams_config_default(C.byref(cfg))
    return cfg


def weights_of(cfg, fill=1.0):
    return (C.c_float * (2 * cfg.n_beams * cfg.n_rx))(*([fill] * (2 * cfg.n_beams * cfg.n_rx)))


def test_layout_and_defaults(lib_built):
    assert C.sizeof(L.FmcwBeamsConfig) == 32
    names = ["n_range", "n_doppler", "n_rx", "n_beams", "window", "mti_mode", "reserved", "device_id"]
    assert [f[0] for f in L.FmcwBeamsConfig._fields_] == names
    for i, name in enumerate(names):
        assert getattr(L.FmcwBeamsConfig, name).offset == 4 * i
    src = L.HEADER_PATH.read_text()
    body = src[src.index("typedef struct fmcw_beams_config {"):src.index("} fmcw_beams_config;")]
    assert [n for n in names if n + ";" in body] == names               # every field, in this order
    assert sorted(names, key=lambda n: body.index(n + ";")) == names
    cfg = default_cfg(lib_built)
    assert (cfg.n_range, cfg.n_doppler, cfg.n_rx, cfg.n_beams) == (1024, 128, 1, 1)
    assert (cfg.window, cfg.mti_mode, cfg.reserved, cfg.device_id) == (L.WIN_HAMMING, L.MTI_OFF, 0, 0)
    assert lib_built.fmcw_abi_version() == 8 and "Still 8 with the beamformer" in src


def test_new_symbols_exported(lib_built):
    out = subprocess.run(["nm", "-D", "--defined-only", str(L.LIB_PATH)], capture_output=True, text=True,
                         check=True).stdout
    src = L.HEADER_PATH.read_text()
    for name in NEW_SYMBOLS:
        assert f" T {name}\n" in out, name
        assert name in L.SIGNATURES and f"{name}(" in src


@pytest.mark.parametrize("field,value,msg", [
    ("n_range", 1000, b"n_range"), ("n_range", 32, b"n_range"), ("n_range", 16384, b"n_range"),
    ("n_doppler", 16, b"n_doppler"), ("n_doppler", 2048, b"n_doppler"), ("n_doppler", 96, b"n_doppler"),
    ("n_rx", 0, b"n_rx"), ("n_rx", 65, b"n_rx"),
    ("n_beams", 0, b"n_beams"), ("n_beams", 65, b"n_beams"),
    ("window", L.WIN_Q15_RTL, b"window"), ("window", 3, b"window"),
    ("mti_mode", 1, b"mti_mode"), ("mti_mode", 4, b"mti_mode"),
    ("reserved", 1, b"reserved"),
    ("device_id", -1, b"device_id"), ("device_id", 64, b"device_id"),
])
def test_create_rejects_bad_fields(lib_built, field, value, msg):
    cfg = default_cfg(lib_built)
    w = (C.c_float * (2 * 65 * 65))(*([1.0] * (2 * 65 * 65)))           # enough for any n_rx, n_beams tried here
    setattr(cfg, field, value)
    h = C.c_void_p(1)
    assert lib_built.fmcw_beams_create(C.byref(cfg), w, C.byref(h)) == L.FMCW_EINVAL
    assert msg in lib_built.fmcw_last_error()
    assert not h.value


# the fields fmcw_beams_create checks through the shared helpers, in its order, each between the field
# checked before it and the one after: (field, bad value, the whole message)
SHARED_CHECKS = [
    ("n_doppler", 16, b"n_doppler=16: must be a power of two in [32, 1024]"),
    ("n_rx", 65, b"n_rx=65: must be in [1, 64]"),
    ("n_beams", 65, b"n_beams=65: must be in [1, 64]"),
    ("window", L.WIN_Q15_RTL, b"window 2: the beamformer has the float windows only (NONE, HAMMING)"),
    ("mti_mode", 4, b"mti_mode 4 (0, 2, 3)"),
    ("reserved", 1, b"reserved 1: must be 0"),
]


@pytest.mark.parametrize("i", [1, 3, 4])
def test_shared_checks_keep_their_text_and_order(lib_built, i):
    """With the field before it bad as well, the earlier message; with the field after it bad as well,
    its own, byte for byte."""
    for lo, want in ((i - 1, SHARED_CHECKS[i - 1][2]), (i, SHARED_CHECKS[i][2])):
        cfg = default_cfg(lib_built)
        for field, value, _ in SHARED_CHECKS[lo:lo + 2]:
            setattr(cfg, field, value)
        w = (C.c_float * (2 * 65 * 65))(*([1.0] * (2 * 65 * 65)))
        h = C.c_void_p(1)
        assert lib_built.fmcw_beams_create(C.byref(cfg), w, C.byref(h)) == L.FMCW_EINVAL
        assert lib_built.fmcw_last_error() == want and not h.value


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -float("inf")])
def test_create_rejects_bad_weights(lib_built, bad):
    cfg = default_cfg(lib_built)
    cfg.n_rx, cfg.n_beams = 3, 2
    for pos in (0, 7, 11):                                              # re of the first, im of beam 1 rx 0, the last
        w = weights_of(cfg)
        w[pos] = bad
        h = C.c_void_p(1)
        assert lib_built.fmcw_beams_create(C.byref(cfg), w, C.byref(h)) == L.FMCW_EINVAL
        err = lib_built.fmcw_last_error()
        assert b"weights" in err and f"beam {pos // 2 // 3}, rx {pos // 2 % 3}".encode() in err
        assert not h.value
    h = C.c_void_p(1)
    assert lib_built.fmcw_beams_create(C.byref(cfg), None, C.byref(h)) == L.FMCW_EINVAL
    assert b"weights" in lib_built.fmcw_last_error() and not h.value


def test_null_arguments(lib_built):
    assert lib_built.fmcw_beams_create(None, None, None) == L.FMCW_EINVAL
    assert lib_built.fmcw_beams_destroy(None) == L.FMCW_OK
    assert lib_built.fmcw_beams_set_grid_for_test(None, 1) == L.FMCW_EINVAL
    assert b"beamformer" in lib_built.fmcw_last_error()
    assert lib_built.fmcw_beams_enqueue(None, None, 1, None, None) == L.FMCW_EINVAL
    lib_built.fmcw_beams_config_default(None)


def test_create_without_device_fails_cleanly(lib_built):
    cfg = default_cfg(lib_built)
    h = C.c_void_p(1)
    rc = lib_built.fmcw_beams_create(C.byref(cfg), weights_of(cfg), C.byref(h))
    if L.device_count() > 0:      # a valid configuration: the GPU tests take it from here
        assert rc == L.FMCW_OK and h.value
        assert lib_built.fmcw_beams_destroy(h) == L.FMCW_OK
    else:
        assert rc == L.FMCW_ENODEV and not h.value


def test_python_class_checks_the_weight_shape(lib_built):
    with pytest.raises(ValueError, match="weights"):
        BeamFormer(64, 32, 4, np.ones((2, 3), np.complex64))
    with pytest.raises(ValueError, match="weights"):
        BeamFormer(64, 32, 4, np.ones(4, np.complex64))


def test_steering_weights():
    nus = [0.25, -0.125, 0.0, 0.5]
    w = steering_weights(4, nus)
    assert w.dtype == np.complex64 and w.shape == (4, 4)
    k = np.arange(4)
    for b, nu in enumerate(nus):
        np.testing.assert_allclose(w[b], np.exp(-2j * np.pi * nu * k) / 4, atol=1e-7)
        assert abs(w[b] @ np.exp(2j * np.pi * nu * k) - 1.0) < 1e-6            # unit gain at its own nu
    # orthogonal beams null each other's plane wave (uniform taper, nu a multiple of 1 / n_rx apart)
    assert abs(w[0] @ np.exp(2j * np.pi * 0.5 * k)) < 1e-6
    t = np.array([0.5, 1.0, 1.0, 0.5])
    wt = steering_weights(4, [0.1], taper=t)
    np.testing.assert_allclose(wt[0], t * np.exp(-2j * np.pi * 0.1 * k) / 3.0, atol=1e-7)
    assert abs(wt[0] @ np.exp(2j * np.pi * 0.1 * k) - 1.0) < 1e-6
    assert steering_weights(1, 0.3).shape == (1, 1) and steering_weights(1, 0.3)[0, 0] == 1
    with pytest.raises(ValueError):
        steering_weights(4, [0.1], taper=[1, 1, 1])
    with pytest.raises(ValueError):
        steering_weights(2, [0.1], taper=[1, -1])


def test_reference_on_a_plane_wave():
    """One noiseless target: the beam at its nu holds n_doppler (window "none") at its cell, an
    orthogonal beam nothing; S there is the same for both."""
    nrx, nc, nr, r, d = 4, 32, 4, 2, 5
    c = np.arange(nc)
    spec = np.zeros((1, nrx, nr, nc), np.complex128)
    for k in range(nrx):
        spec[0, k, r] = np.exp(2j * np.pi * (d * c / nc + 0.25 * k))
    maps, S = R.beams_ref(spec, steering_weights(nrx, [0.25, 0.5]), win="none")
    assert maps.shape == S.shape == (1, 2, nr, nc)
    assert abs(maps[0, 0, r, d] - nc) < 1e-4 and maps[0, 1, r, d] < 1e-4       # the weights are fp32
    assert abs(S[0, 0, r, d] - nc) < 1e-4 and abs(S[0, 1, r, d] - nc) < 1e-4
    assert np.all(maps <= S + 1e-9)
    used = R.assert_maps_match(maps.astype(np.float32), maps, S, label="the reference against itself")
    assert used["peak"] < 0.01 and used["bin"] < 0.01
    with pytest.raises(AssertionError):
        R.assert_maps_match((maps + 2e-4 * S.max()).astype(np.float32), maps, S)


@pytest.mark.parametrize("mti", [0, 2, 3])
def test_reference_one_channel_is_the_oracle_map(mti):
    """n_rx = 1, W = [[1]]: the oracle's single-channel linear map for the same window and MTI mode."""
    cube = synth.frame(64, 32, 1, "two_targets", seed=31)
    want = O.process(cube, None, mti_mode=mti)["mag"]
    maps, S = R.beams_ref(O.range_ct(cube)[None], [[1.0]], mti=mti)
    assert np.abs(maps[0, 0] - want).max() <= 1e-9 * want.max()
    np.testing.assert_allclose(S, maps, rtol=1e-12)


@pytest.mark.parametrize("nc", [32, 1024])
@pytest.mark.parametrize("nrx", [2, 3, 4])
def test_reference_null_and_main_beam(nrx, nc):
    """The null / main beam property the GPU test asserts, on the NumPy reference alone (synth seed
    40): at the first target's peak cell the beam at nu = 0.25 holds the maximum and every beam
    j / n_rx away holds at most 5e-5 of it."""
    nr = 64
    cube = synth.frame(nr, nc, nrx, "two_targets", seed=40, rx_phase=[0.25, -0.125])
    maps, _ = R.beams_ref(O.range_ct(cube)[None], steering_weights(nrx, 0.25 + np.arange(nrx) / nrx))
    cell = maps[0, :, 100 * nr // 1024, 5]
    print(f"\nrx{nrx} 64x{nc}: other beams / beam 0 at the peak cell: {cell[1:] / cell[0]}")
    assert cell.argmax() == 0 and np.all(cell[1:] <= 5e-5 * cell[0])


def test_format_round_trip(tmp_path):
    d = np.zeros(4, DET_DTYPE)
    d["frame"], d["range"], d["doppler"] = [0, 5, 7, 23], [6, 31, 0, 63], [5, 22, 31, 0]
    d["mag"] = np.array([1.2345678e10, 3.5, 0.25, 7.0], np.float32)
    d["threshold"] = np.array([1.5e9, 3.25, 0.125, 6.9999995], np.float32)
    nus = (np.arange(8) - 4) / 8
    assert formats.write_beam_detections(tmp_path / "b.txt", d, nus, spacing=0.25) == 4
    got = formats.read_beam_detections(tmp_path / "b.txt")
    assert got.shape == (4, 8)
    np.testing.assert_array_equal(got[:, 0], d["frame"] // 8)
    np.testing.assert_array_equal(got[:, 1], d["frame"] % 8)
    np.testing.assert_array_equal(got[:, 2:4], np.stack([d["range"], d["doppler"]], 1))
    np.testing.assert_array_equal(got[:, 4].astype(np.float32), d["mag"])          # 9 digits: the fp32 value
    np.testing.assert_array_equal(got[:, 5].astype(np.float32), d["threshold"])
    np.testing.assert_allclose(got[:, 6], nus[d["frame"] % 8], atol=5e-7)
    np.testing.assert_allclose(got[:, 7], nus[d["frame"] % 8] / 0.25, atol=5e-7)
    assert (tmp_path / "b.txt").read_text().splitlines()[1].split()[:4] == ["0", "5", "31", "22"]
    formats.write_beam_detections(tmp_path / "c.txt", d, nus, doppler_centred=True, n_doppler=32)
    np.testing.assert_array_equal(formats.read_beam_detections(tmp_path / "c.txt")[:, 3], (d["doppler"] + 16) % 32)
    with pytest.raises(ValueError):
        formats.write_beam_detections(tmp_path / "d.txt", d, nus, doppler_centred=True)
    assert formats.write_beam_detections(tmp_path / "e.txt", d[:0], nus) == 0
    assert formats.read_beam_detections(tmp_path / "e.txt").shape == (0, 8)


def test_cli_beams_arguments(capsys, tmp_path):
    ap = cli.build_parser()
    assert ap.parse_args(["x.npy"]).beams == 0
    a = ap.parse_args(["x.npy", "--beams", "8", "--rx-spacing", "0.25"])
    assert a.beams == 8 and a.rx_spacing == 0.25 and a.bearings is False
    with pytest.raises(SystemExit):
        ap.parse_args(["x.npy", "--beams", "many"])
    for argv, msg in ((["--beams", "4", "--window", "q15_rtl"], "float window"),
                      (["--beams", "65"], "1..64"), (["--beams", "-1"], "1..64"),
                      (["--beams", "4", "--rx-spacing", "0"], "--rx-spacing"),
                      (["--beams", "4", "--cfar", "none"], "CFAR")):
        with pytest.raises(SystemExit):
            cli.main(["x.npy"] + argv)                                   # rejected before the input is read
        assert msg in capsys.readouterr().err
    np.save(tmp_path / "one_rx.npy", synth.frames(1, 64, 32, 1))
    with pytest.raises(SystemExit):                                      # rejected before any device access
        cli.main([str(tmp_path / "one_rx.npy"), "--n-range", "64", "--n-doppler", "32", "--beams", "4"])
    assert "multi-rx" in capsys.readouterr().err


# ---- what the tolerance leaves unchecked: the scenes the GPU cases run on ---------------------------------
SHARE_CAP = 0.02
FS_CASES = ([(nc, nrx, mti, R.FS_NB) for nc in R.FS_DOPPLERS for nrx in R.FS_RXS for mti in R.FS_MTIS] +
            [(32, nrx, 0, nb) for nrx, nb in R.FS_LIMITS])


def fmt_shares(sh):
    return ", ".join(f"{k} {100 * v:.3f} %" for k, v in sh.items())


@pytest.mark.parametrize("nc,nrx,mti,nb", FS_CASES)
def test_full_scale_scene_is_checked_in_every_cell(nc, nrx, mti, nb):
    """On every full-scale case of tests/test_gpu_beams.py a map of zeros, the reference one range row
    off and the reference of the next frame or beam each pass assert_maps_match's bounds in at most
    2 % of the cells (what is left is the canceller's null at Doppler 0, and chance).  Measured on the
    reference alone, before any GPU value."""
    spec, w, win = R.full_scale_case(nc, nrx, mti, nb)
    assert spec.dtype == np.complex64 and spec.shape == (R.FS_NF, nrx, R.FS_NR, nc)
    rms = np.sqrt(np.mean(spec.real.astype(np.float64) ** 2)), np.sqrt(np.mean(spec.imag.astype(np.float64) ** 2))
    assert np.allclose(rms, R.FULL_SCALE_RMS, rtol=0.05), rms
    sh = R.unchecked_shares(*R.beams_ref(spec, w, win, mti))
    print(f"\nfull scale {R.FS_NR}x{nc} rx{nrx} beams{nb} mti{mti} {win}: passes unnoticed in {fmt_shares(sh)}")
    assert max(sh.values()) <= SHARE_CAP, sh


def two_targets_case(nc, nrx=4, nr=64, nf=R.FS_NF, seed=40):
    """The scene of the GPU cases before the full-scale one: synth's two_targets through the oracle's
    range stage (fmcw_oracle.range_ct, fp64) as the host stand-in for fmcw_range_ct, rounded to the
    complex64 the GPU stage writes; 3 random beams."""
    cube = synth.frames(nf, nr, nc, nrx, "two_targets", seed=seed, rx_phase=[0.25, -0.125])
    spec = O.range_ct(cube).astype(np.complex64)
    rng = np.random.default_rng(seed)
    w = (rng.standard_normal((3, nrx)) + 1j * rng.standard_normal((3, nrx))).astype(np.complex64)
    return spec, w


def test_two_targets_scene_is_unchecked_in_most_cells():
    """Why the full-scale scene exists: on two_targets at 64 x 1024 with MTI off a map of zeros passes
    both bounds in more than 90 % of the cells."""
    spec, w = two_targets_case(1024)
    sh = R.unchecked_shares(*R.beams_ref(spec, w, "hamming", 0))
    print(f"\ntwo_targets 64x1024 rx4 beams3 mti0 hamming: passes unnoticed in {fmt_shares(sh)}")
    assert sh["zero"] > 0.90, sh


def test_unchecked_share_counts_both_bounds():
    """unchecked_share on a hand-made pair: a cell passes when it is within 1e-4 of the map's largest
    scale and, above 1e-3 of that scale, within 1e-4 of its own."""
    ref = np.array([[[[1000.0, 500.0, 0.5, 0.05]]]])
    S = ref.copy()
    assert R.unchecked_share(ref, S, ref) == 1.0
    assert R.unchecked_share(ref, S, 0.0) == 0.25                    # only 0.05 is below 1e-4 * 1000
    other = ref + np.array([0.09, 0.06, 0.09, 0.09])                # 0.06 > 1e-4 * 500: the per-bin bound
    assert R.unchecked_share(ref, S, other) == 0.75
    assert R.unchecked_share(ref, S, ref + 0.11) == 0.0              # the peak bound, everywhere
    S2 = np.array([[[[1000.0, 500.0, 2.0, 0.05]]]])                  # 2.0 > 1e-3 * 1000: now held to 2e-4
    assert R.unchecked_share(ref, S2, other) == 0.5


# ---- a catalogue of kernel defects, modelled on the reference ------------------------------------------
def model(spec, w, win, mti, *, delay="zero", keep_x2_at_chirp_1=False, win_shift=0):
    """beams_ref's maps with the canceller's edge and the window open to a defect."""
    x = np.einsum("bk,fkrc->fbrc", np.asarray(w).astype(np.complex128), np.asarray(spec).astype(np.complex128))
    nc = x.shape[-1]

    def delayed(k):
        if delay == "zero":
            return R._delayed(x, k)
        flat = x.reshape(x.shape[:2] + (-1,))                         # the row before it in memory
        return R._delayed(flat, k).reshape(x.shape)
    m1, m2 = R.MTI_COEF[mti]
    x1, x2 = delayed(1), delayed(2)
    if keep_x2_at_chirp_1:
        x2[..., 1] = x[..., 1]                                         # the clamped load's value, not dropped
    y = x - m1 * x1 + m2 * x2
    return np.abs(np.fft.fft(y * np.roll(R.window(nc, win), win_shift), axis=-1))


def defect_row(spec, w, win, mti):
    m = model(spec, w, win, mti)
    m[-1, :, -1] = m[-1, :, -2]
    return m


def defect_frame(spec, w, win, mti):
    m = model(spec, w, win, mti)
    m[1:] = m[0]
    return m


# name -> (the defective maps, the MTI modes in which the defect changes anything)
DEFECTS = {
    "one row of the last tile taken from the row before": (defect_row, (0, 2, 3)),
    "frame f > 0 computed from frame 0": (defect_frame, (0, 2, 3)),
    "beam b > 0 accumulated onto beam b-1's sum":
        (lambda s, w, win, mti: model(s, np.cumsum(np.asarray(w, np.complex128), axis=0), win, mti), (0, 2, 3)),
    "the delay line before chirp 0 taken from the preceding row":
        (lambda s, w, win, mti: model(s, w, win, mti, delay="memory"), (2, 3)),
    "x[c-2] not dropped at chirp 1": (lambda s, w, win, mti: model(s, w, win, mti, keep_x2_at_chirp_1=True), (3,)),
    "a conjugated weight": (lambda s, w, win, mti: model(s, np.conj(w), win, mti), (0, 2, 3)),
    "the last channel left out":
        (lambda s, w, win, mti: model(s, np.concatenate([w[:, :-1], 0 * w[:, -1:]], 1), win, mti), (0, 2, 3)),
    "the window shifted by one chirp": (lambda s, w, win, mti: model(s, w, win, mti, win_shift=1), (0, 2, 3)),
}


def seen(defect, spec, w, mti):
    """(whether assert_maps_match tells the defective maps, rounded to the fp32 a kernel writes, from
    the reference; the share of the cells the defect changes in which a bound is exceeded)."""
    ref, S = R.beams_ref(spec, w, "hamming", mti)
    bad = defect(spec, w, "hamming", mti).astype(np.float32)
    changed = bad != ref.astype(np.float32)
    assert changed.any()
    caught = changed & ~R.passes(ref, S, bad)
    assert caught.any() == (max(R.bounds_used(bad, ref, S).values()) > 1.0)
    return bool(caught.any()), caught.sum() / changed.sum()


def test_the_defect_model_without_a_defect_is_the_reference():
    spec, w, _ = R.full_scale_case(32, 4, 3)
    for win in ("hamming", "none"):
        for mti in (0, 2, 3):
            assert np.array_equal(model(spec, w, win, mti), R.beams_ref(spec, w, win, mti)[0])


@pytest.mark.parametrize("name", list(DEFECTS))
@pytest.mark.parametrize("nc", [32, 1024])
def test_full_scale_scene_rejects_the_defect(nc, name):
    """Each defect, in every MTI mode in which it changes anything (Hamming, 4 rx, 3 random beams,
    2 frames), fails assert_maps_match on the full-scale scene."""
    defect, mtis = DEFECTS[name]
    for mti in mtis:
        spec, w, _ = R.full_scale_case(nc, 4, mti)
        rejected, share = seen(defect, spec, w, mti)
        print(f"\nfull scale 64x{nc} mti{mti}: {name}: out of bound in {100 * share:.1f} % of the cells it changes")
        assert rejected, f"{name}: passes at n_doppler {nc}, mti {mti}"
        with pytest.raises(AssertionError):
            R.assert_maps_match(defect(spec, w, "hamming", mti).astype(np.float32), *R.beams_ref(spec, w, "hamming", mti))


@pytest.mark.parametrize("nc", [32, 1024])
def test_which_defects_the_two_targets_scene_lets_through(nc):
    """The same catalogue on the two_targets scene.  Information, not an assertion: which defects the
    scene of the other GPU cases lets through under the same bounds, and in how few of the cells a
    defect changes it is seen at all (a defect confined to the other cells passes)."""
    spec, w = two_targets_case(nc)
    print()
    for name, (defect, mtis) in DEFECTS.items():
        for mti in mtis:
            rejected, share = seen(defect, spec, w, mti)
            print(f"two_targets 64x{nc} mti{mti}: {name}: {'rejected' if rejected else 'PASSES UNNOTICED'}, "
                  f"out of bound in {100 * share:.2f} % of the cells it changes")


@pytest.mark.parametrize("nc,nrx,mti,nb", FS_CASES)
def test_float32_evaluation_of_the_full_scale_cases(nc, nrx, mti, nb):
    """beams_ref.beams_f32 (the specification in float32 on the CPU) against the fp64 reference: the
    fractions of the two bounds that rounding alone uses, for DESIGN.md 4c to set beside the GPU's.
    The peak bound is asserted with a wide margin; the per-bin figure is printed (a matrix DFT's
    rounding is not the kernel's)."""
    spec, w, win = R.full_scale_case(nc, nrx, mti, nb)
    used = R.bounds_used(R.beams_f32(spec, w, win, mti), *R.beams_ref(spec, w, win, mti))
    print(f"\nfloat32 on the CPU, {R.FS_NR}x{nc} rx{nrx} beams{nb} mti{mti} {win}: peak {used['peak']:.3g}, bin {used['bin']:.3g}")
    assert used["peak"] <= 0.05
