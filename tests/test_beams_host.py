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
