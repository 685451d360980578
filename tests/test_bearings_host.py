"""The bearing estimator without a GPU: its specification (tests/bearings_ref.py) against closed
forms and against the oracle's NCI map, the synthetic generator's new rx_phase argument, the C-ABI's
argument checks (they come before any device access), the text format and the CLI's arguments."""
import ctypes as C
import hashlib
import json

import numpy as np
import pytest

import fmcw_oracle as O
from conftest import GOLDEN
from fmcw import _lib as L
from fmcw import BEARING_DTYPE, BearingEstimator, DET_DTYPE, PLOT_DTYPE, cli, formats, synth  # noqa: F401
import bearings_ref as R


def plane_wave(phases, nrx=4, nc=32, nr=4, r=2, d=5, amps=None):
    """A noiseless spectrum [1][rx][range][chirp]: targets in cell (r, d) at the given rx phases."""
    amps = amps or [1.0] * len(phases)
    c = np.arange(nc)
    spec = np.zeros((1, nrx, nr, nc), np.complex128)
    for p, a in zip(phases, amps):
        for k in range(nrx):
            spec[0, k, r] += a * np.exp(2j * np.pi * (d * c / nc + p * k))
    rec = np.zeros(1, DET_DTYPE)
    rec["range"], rec["doppler"] = r, d
    return spec, rec


@pytest.mark.parametrize("p", [0.25, 0.125, -0.25, -0.4, 0.0, 0.49])
@pytest.mark.parametrize("win", ["hamming", "none"])
def test_plane_wave_gives_its_phase(p, win):
    spec, rec = plane_wave([p])
    out, s, _ = R.bearings_ref(spec, rec, win=win)
    assert abs(out["nu"][0] - p) < 1e-12 and abs(out["coherence"][0] - 1.0) < 1e-12
    assert abs(out["sin_theta"][0] - p / 0.5) < 1e-12 and out["flags"][0] == 0
    assert abs(out["power"][0] - np.sqrt(4) * R.window(32, win).sum()) < 1e-9


def test_two_targets_in_one_cell_lower_coherence():
    spec, rec = plane_wave([0.2, -0.2])
    out, _, _ = R.bearings_ref(spec, rec)
    assert out["coherence"][0] < 0.9
    one, _, _ = R.bearings_ref(*plane_wave([0.2]))
    assert one["coherence"][0] > 1 - 1e-12


def test_one_rx_sets_flag_2():
    spec, rec = plane_wave([0.25], nrx=1)
    out, s, _ = R.bearings_ref(spec, rec)
    assert out["flags"][0] == R.FLAG_ONE_RX and out["nu"][0] == 0 and out["coherence"][0] == 0
    assert out["power"][0] == pytest.approx(abs(s[0, 0]))


def test_spacing_quarter_nu_03_sets_flag_1():
    spec, rec = plane_wave([0.3])
    out, _, _ = R.bearings_ref(spec, rec, spacing=0.25)
    assert out["flags"][0] == R.FLAG_NO_ANGLE and out["sin_theta"][0] == pytest.approx(1.2)
    assert R.bearings_ref(spec, rec, spacing=0.5)[0]["flags"][0] == 0


def test_out_of_range_records_read_nothing():
    spec, rec = plane_wave([0.25])
    recs = np.repeat(rec, 4)
    recs["frame"][1], recs["range"][2], recs["doppler"][3] = 1, 4, 32
    out, s, a = R.bearings_ref(spec, recs)
    assert list(out["flags"]) == [0, 4, 4, 4]
    assert not np.any(s[1:]) and not np.any(a[1:]) and not np.any(out["power"][1:])


@pytest.mark.parametrize("mti", [0, 2, 3])
@pytest.mark.parametrize("geom", [(64, 32, 4), (128, 64, 2), (64, 128, 3)])
def test_power_is_the_oracle_map_cell(geom, mti):
    """With the path's own window and MTI mode, sqrt(sum_k |s_k|^2) is the oracle's NCI map cell, at
    every oracle detection (1-D CFAR), to 1e-9 of the frame peak."""
    ns, nc, nrx = geom
    cube = synth.frame(ns, nc, nrx, "two_targets", seed=31)
    o = O.process(cube, O.Cfar1D(), mti_mode=mti)
    dets = o["dets"]
    assert len(dets) > 10
    spec = O.range_ct(cube)[None]        # [1][rx][range][chirp]
    out, _, _ = R.bearings_ref(spec, dets, mti=mti)
    want = o["mag"][dets["range"], dets["doppler"]]
    assert np.abs(out["power"] - want).max() <= 1e-9 * o["mag"].max()


@pytest.mark.parametrize("mti", R.FS_MTIS)
@pytest.mark.parametrize("nc", R.FS_DOPPLERS)
def test_full_scale_list_visits_every_row_and_bin(nc, mti):
    """The full-scale cases of tests/test_gpu_bearings.py on the reference alone: the list holds every
    (frame, range row) 8 times and every Doppler bin, and the reference rounded to the record's fp32
    fields passes assert_bearings_match -- so at most 5 % of the list is ill-conditioned for nu (white
    cells have no preferred phase slope, and the canceller's null takes the records at Doppler 0)."""
    spec, recs, win = R.full_scale_case(nc, mti)
    assert len(recs) == R.FS_NF * R.FS_NR * R.FS_BINS
    rows = set(zip(recs["frame"].tolist(), recs["range"].tolist()))
    assert len(rows) == R.FS_NF * R.FS_NR and set(recs["doppler"].tolist()) == set(range(nc))
    ref, s, a = R.bearings_ref(spec, recs, win=win, mti=mti)
    got = np.zeros(len(recs), BEARING_DTYPE)
    for k in ("frame", "range", "doppler", "flags", "nu", "power", "coherence"):
        got[k] = ref[k]
    got["sin_theta"] = got["nu"] * np.float32(2.0)
    used = R.assert_bearings_match(got, s.astype(np.complex64), ref, s, a, label="the reference against itself")
    print(f"\nfull scale {R.FS_NR}x{nc} rx{R.FS_NRX} mti{mti} {win}: {len(recs)} records, {used['skipped']} "
          f"ill-conditioned for nu, worst E_P / |P| among the rest {used['cond']:.3g}")
    assert used["s"] <= 0.05 and used["power"] <= 0.05


def test_detections_of_two_targets_sit_at_a_quarter_cycle():
    cube = synth.frame(64, 32, 4, "two_targets", seed=1234)
    o = O.process(cube, O.Cfar1D())
    out, _, _ = R.bearings_ref(O.range_ct(cube)[None], o["dets"])
    assert np.mean(np.abs(out["nu"] - 0.25) < 0.01) > 0.9


def test_synth_default_is_byte_identical():
    """rx_phase's default reproduces the arrays the generator gave before it had the argument
    (tests/golden/synth_default.npz and the SHA-256 of larger ones): the bench and every other test
    draw from it."""
    g = np.load(GOLDEN / "synth_default.npz")
    for recipe in ("two_targets", "random_target"):
        for dt in ("f32", "i16", "f16"):
            got = synth.frames(2, 32, 16, 3, recipe, seed=1234, dtype=dt)
            want = g[f"{recipe}_{dt}"]
            assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), (recipe, dt)
            assert synth.frames(2, 32, 16, 3, recipe, seed=1234, dtype=dt, rx_phase=0.25).tobytes() == want.tobytes()
    assert synth.frame(32, 16).tobytes() == g["frame_two_targets_1rx"].tobytes()
    h = json.loads((GOLDEN / "synth_default_sha256.json").read_text())
    for recipe in ("two_targets", "random_target"):
        got = synth.frames(2, 256, 64, 4, recipe, seed=1234)
        assert hashlib.sha256(got.tobytes()).hexdigest() == h[f"{recipe}_256x64x4"]
    got = synth.frames(1, 512, 128, 1, "two_targets", seed=7, dtype="i16")
    assert hashlib.sha256(got.tobytes()).hexdigest() == h["two_targets_512x128x1_i16"]


def test_synth_rx_phase():
    a = synth.frame(64, 32, 4, "two_targets", seed=5)
    b = synth.frame(64, 32, 4, "two_targets", seed=5, rx_phase=[0.125, -0.25])
    assert np.array_equal(a[0], b[0]) and not np.array_equal(a[1], b[1])      # channel 0 has no offset
    assert np.array_equal(synth.frame(64, 32, 4, "two_targets", seed=5, rx_phase=[0.25, 0.25]), a)
    with pytest.raises(ValueError, match="rx_phase"):
        synth.frame(64, 32, 4, "two_targets", rx_phase=[0.1])
    o = O.process(b, O.Cfar1D())
    spec = O.range_ct(b)[None]
    rec = np.zeros(2, DET_DTYPE)
    rec["range"], rec["doppler"] = [100 * 64 // 1024, 500 * 64 // 1024], [5, 32 - 10]
    out, _, _ = R.bearings_ref(spec, rec)
    assert o["mag"].max() > 0
    assert abs(out["nu"][0] - 0.125) < 0.01 and abs(out["nu"][1] + 0.25) < 0.01


def default_cfg(lib):
    cfg = L.FmcwBearingsConfig()
    lib.fmcw_bearings_config_default(C.byref(cfg))
    return cfg


def test_layouts_and_defaults(lib_built):
    assert C.sizeof(L.FmcwBearing) == 32 == BEARING_DTYPE.itemsize and C.sizeof(L.FmcwBearingsConfig) == 32
    for name in BEARING_DTYPE.names:
        assert BEARING_DTYPE.fields[name][1] == getattr(L.FmcwBearing, name).offset
    cfg = default_cfg(lib_built)
    assert (cfg.n_range, cfg.n_doppler, cfg.n_rx, cfg.window, cfg.mti_mode) == (1024, 128, 1, L.WIN_HAMMING, L.MTI_OFF)
    assert (cfg.spacing, cfg.max_records, cfg.device_id) == (0.5, 1 << 20, 0)
    src = L.HEADER_PATH.read_text()
    assert "#define FMCW_BEARING_STATUS_WORDS 2" in src and L.BEARING_STATUS_WORDS == 2
    for name, v in (("NO_ANGLE", L.BEARING_NO_ANGLE), ("ONE_RX", L.BEARING_ONE_RX), ("OUT_OF_RANGE", L.BEARING_OUT_OF_RANGE)):
        assert f"#define FMCW_BEARING_{name} {v}u" in src
    assert (R.FLAG_NO_ANGLE, R.FLAG_ONE_RX, R.FLAG_OUT_OF_RANGE) == (1, 2, 4)
    assert lib_built.fmcw_abi_version() == 8


@pytest.mark.parametrize("field,value,msg", [
    ("n_range", 1000, b"n_range"), ("n_range", 32, b"n_range"), ("n_range", 16384, b"n_range"),
    ("n_doppler", 16, b"n_doppler"), ("n_doppler", 2048, b"n_doppler"), ("n_doppler", 96, b"n_doppler"),
    ("n_rx", 0, b"n_rx"), ("n_rx", 65, b"n_rx"),
    ("window", L.WIN_Q15_RTL, b"window"), ("window", 3, b"window"),
    ("mti_mode", 1, b"mti_mode"), ("mti_mode", 4, b"mti_mode"),
    ("spacing", 0.0, b"spacing"), ("spacing", -0.5, b"spacing"), ("spacing", float("nan"), b"spacing"),
    ("spacing", float("inf"), b"spacing"),
    ("max_records", 0, b"max_records"), ("max_records", 1 << 31, b"max_records"),
    ("device_id", -1, b"device_id"), ("device_id", 64, b"device_id"),
])
def test_create_rejects_bad_fields(lib_built, field, value, msg):
    cfg = default_cfg(lib_built)
    setattr(cfg, field, value)
    h = C.c_void_p(1)
    assert lib_built.fmcw_bearings_create(C.byref(cfg), C.byref(h)) == L.FMCW_EINVAL
    assert msg in lib_built.fmcw_last_error()
    assert not h.value


# the fields fmcw_bearings_create checks through the shared helpers, in its order, each between the field
# checked before it and the one after: (field, bad value, the whole message)
SHARED_CHECKS = [
    ("n_doppler", 16, b"n_doppler=16: must be a power of two in [32, 1024]"),
    ("n_rx", 65, b"n_rx=65: must be in [1, 64]"),
    ("window", L.WIN_Q15_RTL, b"window 2: the bearing estimator has the float windows only (NONE, HAMMING)"),
    ("mti_mode", 1, b"mti_mode 1 (0, 2, 3)"),
    ("spacing", -0.5, b"spacing -0.5: must be positive and finite (wavelengths)"),
]


@pytest.mark.parametrize("i", [1, 2, 3])
def test_shared_checks_keep_their_text_and_order(lib_built, i):
    """With the field before it bad as well, the earlier message; with the field after it bad as well,
    its own, byte for byte."""
    for lo, want in ((i - 1, SHARED_CHECKS[i - 1][2]), (i, SHARED_CHECKS[i][2])):
        cfg = default_cfg(lib_built)
        for field, value, _ in SHARED_CHECKS[lo:lo + 2]:
            setattr(cfg, field, value)
        h = C.c_void_p(1)
        assert lib_built.fmcw_bearings_create(C.byref(cfg), C.byref(h)) == L.FMCW_EINVAL
        assert lib_built.fmcw_last_error() == want and not h.value


def test_null_and_stride_arguments(lib_built):
    assert lib_built.fmcw_bearings_create(None, None) == L.FMCW_EINVAL
    assert lib_built.fmcw_bearings_destroy(None) == L.FMCW_OK
    assert lib_built.fmcw_bearings_set_grid_for_test(None, 1) == L.FMCW_EINVAL
    assert b"bearing estimator" in lib_built.fmcw_last_error()
    assert lib_built.fmcw_bearings_enqueue(None, None, 1, None, 16, 0, None, None, None, None, None) == L.FMCW_EINVAL
    lib_built.fmcw_bearings_config_default(None)


def test_create_without_device_fails_cleanly(lib_built):
    cfg = default_cfg(lib_built)
    h = C.c_void_p(1)
    rc = lib_built.fmcw_bearings_create(C.byref(cfg), C.byref(h))
    if L.device_count() > 0:      # a valid configuration: the GPU tests take it from here
        assert rc == L.FMCW_OK and h.value
        assert lib_built.fmcw_bearings_destroy(h) == L.FMCW_OK
    else:
        assert rc == L.FMCW_ENODEV and not h.value


def test_new_symbols_exported(lib_built):
    import subprocess
    out = subprocess.run(["nm", "-D", "--defined-only", str(L.LIB_PATH)], capture_output=True, text=True,
                         check=True).stdout
    for name in ("fmcw_bearings_config_default", "fmcw_bearings_create", "fmcw_bearings_destroy",
                 "fmcw_bearings_enqueue", "fmcw_bearings_set_grid_for_test"):
        assert f" T {name}\n" in out, name
        assert name in L.SIGNATURES


def test_format_round_trip(tmp_path):
    b = np.zeros(3, BEARING_DTYPE)
    b["frame"], b["range"], b["doppler"] = [0, 1, 2], [6, 31, 0], [5, 22, 31]
    b["power"] = np.array([1.2345678e10, 3.5, 0.0], np.float32)
    b["nu"], b["sin_theta"] = [0.125, -0.25, 0.0], [0.25, -0.5, 0.0]
    b["coherence"], b["flags"] = [0.999999, 0.5, 0.0], [0, 1, 4]
    assert formats.write_bearings(tmp_path / "b.txt", b) == 3
    got = formats.read_bearings(tmp_path / "b.txt")
    assert got.shape == (3, 8)
    np.testing.assert_array_equal(got[:, :3], np.stack([b["frame"], b["range"], b["doppler"]], 1))
    np.testing.assert_array_equal(got[:, 3].astype(np.float32), b["power"])     # 9 digits: the fp32 value
    for col, k in ((4, "nu"), (5, "sin_theta"), (6, "coherence")):
        np.testing.assert_allclose(got[:, col], b[k], atol=5e-7)                # 6 decimals
    np.testing.assert_array_equal(got[:, 7], b["flags"])
    formats.write_bearings(tmp_path / "c.txt", b, doppler_centred=True, n_doppler=32)
    np.testing.assert_array_equal(formats.read_bearings(tmp_path / "c.txt")[:, 2], (b["doppler"] + 16) % 32)
    assert (tmp_path / "b.txt").read_text().splitlines()[0].split()[:3] == ["0", "6", "5"]


def test_cli_bearings_arguments(capsys):
    ap = cli.build_parser()
    a = ap.parse_args(["x.npy"])
    assert a.bearings is False and a.rx_spacing == 0.5
    a = ap.parse_args(["x.npy", "--bearings"])
    assert a.bearings is True and a.rx_spacing == 0.5 and a.plots is False
    a = ap.parse_args(["x.npy", "--bearings", "--rx-spacing", "0.25", "--plots"])
    assert a.bearings and a.rx_spacing == 0.25 and a.plots
    with pytest.raises(SystemExit):
        ap.parse_args(["x.npy", "--rx-spacing", "wide"])
    with pytest.raises(SystemExit):
        cli.main(["x.npy", "--bearings", "--window", "q15_rtl"])      # rejected before the input is read
    assert "float window" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        cli.main(["x.npy", "--bearings", "--rx-spacing", "0"])
