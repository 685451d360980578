"""The adaptive beam weights without a GPU: the C-ABI's layout, exports and argument checks (they come
before any device access), the specification (tests/adapt_ref.py) against closed forms, the jammer
scene's margins through tests/beams_ref.py and the oracle's 2-D OS-CFAR, the GPU tests' inputs
against the bound they are held to, and the CLI's arguments."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import fmcw_oracle as O
from fmcw import _lib as L
from fmcw import cli, steering_vectors, steering_weights
import adapt_ref as AR
from beams_ref import beams_ref

NEW_SYMBOLS = ("fmcw_adapt_config_default", "fmcw_adapt_create", "fmcw_adapt_destroy", "fmcw_adapt_enqueue",
               "fmcw_adapt_set_grid_for_test", "fmcw_beams_set_weights_dev")


def default_cfg(lib):
    cfg = L.FmcwAdaptConfig()
    lib.fmcw_adapt_config_default(C.byref(cfg))
    return cfg


def constraints_of(cfg, fill=1.0):
    return (C.c_float * (2 * cfg.n_beams * cfg.n_rx))(*([fill] * (2 * cfg.n_beams * cfg.n_rx)))


def test_layout_and_defaults(lib_built):
    assert C.sizeof(L.FmcwAdaptConfig) == 40
    names = ["n_range", "n_doppler", "n_rx", "n_beams", "mti_mode", "train_r0", "train_rows", "loading", "reserved",
             "device_id"]
    assert [f[0] for f in L.FmcwAdaptConfig._fields_] == names
    for i, name in enumerate(names):
        assert getattr(L.FmcwAdaptConfig, name).offset == 4 * i
    src = L.HEADER_PATH.read_text()
    body = src[src.index("typedef struct fmcw_adapt_config {"):src.index("} fmcw_adapt_config;")]
    assert sorted(names, key=lambda n: body.index(" " + n + ";")) == names
    cfg = default_cfg(lib_built)
    assert (cfg.n_range, cfg.n_doppler, cfg.n_rx, cfg.n_beams) == (1024, 128, 1, 1)
    assert (cfg.mti_mode, cfg.train_r0, cfg.train_rows, cfg.reserved, cfg.device_id) == (L.MTI_OFF, 0, 1024, 0, 0)
    assert cfg.loading == np.float32(1e-2)
    assert lib_built.fmcw_abi_version() == 8 and "Still 8 with the adaptive beam weights" in src
    assert "#define FMCW_ADAPT_INFO_WORDS 8" in src and "#define FMCW_ADAPT_PIVOT_MIN 1e-8 " in src and AR.PIVOT_MIN == 1e-8
    assert "17..64" in body                                            # the header says what is not built


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
    ("n_rx", 0, b"n_rx"), ("n_rx", 17, b"n_rx"),
    ("n_beams", 0, b"n_beams"), ("n_beams", 65, b"n_beams"),
    ("mti_mode", 1, b"mti_mode"), ("mti_mode", 4, b"mti_mode"),
    ("train_rows", 0, b"train_rows"), ("train_rows", 1025, b"train_rows"),
    ("train_r0", 1, b"train_r0"), ("train_r0", 1024, b"train_r0"), ("train_r0", 0xffffffff, b"train_r0"),
    ("loading", -1e-3, b"loading"), ("loading", float("nan"), b"loading"), ("loading", float("inf"), b"loading"),
    ("reserved", 1, b"reserved"),
    ("device_id", -1, b"device_id"), ("device_id", 64, b"device_id"),
])
def test_create_rejects_bad_fields(lib_built, field, value, msg):
    cfg = default_cfg(lib_built)
    a = (C.c_float * (2 * 65 * 17))(*([1.0] * (2 * 65 * 17)))            # enough for any n_rx, n_beams tried here
    setattr(cfg, field, value)
    h = C.c_void_p(1)
    assert lib_built.fmcw_adapt_create(C.byref(cfg), a, C.byref(h)) == L.FMCW_EINVAL
    assert msg in lib_built.fmcw_last_error()
    assert not h.value


# the fields fmcw_adapt_create checks through the shared helpers, in its order, each between the field
# checked before it and the one after: (field, bad value, the whole message)
SHARED_CHECKS = [
    ("n_doppler", 16, b"n_doppler=16: must be a power of two in [32, 1024]"),
    ("n_rx", 17, b"n_rx=17: must be in [1, 16] (17..64 is not built)"),
    ("n_beams", 65, b"n_beams=65: must be in [1, 64]"),
    ("mti_mode", 1, b"mti_mode 1 (0, 2, 3)"),
    ("train_rows", 0, b"train_rows=0: must be in [1, n_range = 1024]"),
]


@pytest.mark.parametrize("i", [1, 3])
def test_shared_checks_keep_their_text_and_order(lib_built, i):
    """With the field before it bad as well, the earlier message; with the field after it bad as well,
    its own, byte for byte."""
    for lo, want in ((i - 1, SHARED_CHECKS[i - 1][2]), (i, SHARED_CHECKS[i][2])):
        cfg = default_cfg(lib_built)
        for field, value, _ in SHARED_CHECKS[lo:lo + 2]:
            setattr(cfg, field, value)
        a = (C.c_float * (2 * 65 * 17))(*([1.0] * (2 * 65 * 17)))
        h = C.c_void_p(1)
        assert lib_built.fmcw_adapt_create(C.byref(cfg), a, C.byref(h)) == L.FMCW_EINVAL
        assert lib_built.fmcw_last_error() == want and not h.value


def test_training_window_inside_the_map(lib_built):
    """[train_r0, train_r0 + train_rows) at the map's last row is accepted as far as the device; one
    row further is FMCW_EINVAL."""
    cfg = default_cfg(lib_built)
    cfg.n_range, cfg.train_r0, cfg.train_rows = 64, 60, 5
    h = C.c_void_p(1)
    assert lib_built.fmcw_adapt_create(C.byref(cfg), constraints_of(cfg), C.byref(h)) == L.FMCW_EINVAL
    assert b"train_r0" in lib_built.fmcw_last_error() and not h.value
    cfg.train_rows = 4
    rc = lib_built.fmcw_adapt_create(C.byref(cfg), constraints_of(cfg), C.byref(h))
    assert rc == (L.FMCW_OK if L.device_count() > 0 else L.FMCW_ENODEV)
    if h.value:
        lib_built.fmcw_adapt_destroy(h)


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -float("inf")])
def test_create_rejects_bad_constraints(lib_built, bad):
    cfg = default_cfg(lib_built)
    cfg.n_rx, cfg.n_beams = 3, 2
    for pos in (0, 7, 11):                                              # re of the first, im of beam 1 rx 0, the last
        a = constraints_of(cfg)
        a[pos] = bad
        h = C.c_void_p(1)
        assert lib_built.fmcw_adapt_create(C.byref(cfg), a, C.byref(h)) == L.FMCW_EINVAL
        err = lib_built.fmcw_last_error()
        assert b"a_host" in err and f"beam {pos // 2 // 3}, rx {pos // 2 % 3}".encode() in err
        assert not h.value
    a = constraints_of(cfg)
    for i in range(6, 12):                                              # beam 1 all zero (-0.0 included)
        a[i] = -0.0 if i % 2 else 0.0
    h = C.c_void_p(1)
    assert lib_built.fmcw_adapt_create(C.byref(cfg), a, C.byref(h)) == L.FMCW_EINVAL
    err = lib_built.fmcw_last_error()
    assert b"a_host" in err and b"beam 1" in err and b"zero" in err and not h.value
    h = C.c_void_p(1)
    assert lib_built.fmcw_adapt_create(C.byref(cfg), None, C.byref(h)) == L.FMCW_EINVAL
    assert b"a_host" in lib_built.fmcw_last_error() and not h.value


def test_null_arguments(lib_built):
    assert lib_built.fmcw_adapt_create(None, None, None) == L.FMCW_EINVAL
    assert lib_built.fmcw_adapt_destroy(None) == L.FMCW_OK
    assert lib_built.fmcw_adapt_set_grid_for_test(None, 1) == L.FMCW_EINVAL
    assert b"adaptive" in lib_built.fmcw_last_error()
    assert lib_built.fmcw_adapt_enqueue(None, None, 1, None, None, None, None) == L.FMCW_EINVAL
    assert lib_built.fmcw_beams_set_weights_dev(None, None, None) == L.FMCW_EINVAL
    assert b"beamformer" in lib_built.fmcw_last_error()
    lib_built.fmcw_adapt_config_default(None)


def test_create_without_device_fails_cleanly(lib_built):
    cfg = default_cfg(lib_built)
    h = C.c_void_p(1)
    rc = lib_built.fmcw_adapt_create(C.byref(cfg), constraints_of(cfg), C.byref(h))
    if L.device_count() > 0:      # a valid configuration: the GPU tests take it from here
        assert rc == L.FMCW_OK and h.value
        assert lib_built.fmcw_adapt_destroy(h) == L.FMCW_OK
    else:
        assert rc == L.FMCW_ENODEV and not h.value


# ---- the reference's own properties ---------------------------------------------------------------
def test_unit_gain_and_white_noise():
    """W a = 1 to 1e-12 for steering and random constraints on a coloured R; R = I (any loading) gives
    the conventional weights, which are steering_weights for a steering vector."""
    for nrx in (1, 2, 5, 8, 16):
        spec = AR.noise_scene(32, nrx)
        for a in AR.case_constraints(nrx, 4, seed=nrx):
            ref = AR.adapt_ref(spec, a, 1e-3, mti=2, train_r0=3, train_rows=20)
            gain = np.einsum("bk,bk->b", ref["W"], a.astype(np.complex128))
            assert np.abs(gain - 1.0).max() <= 1e-12 and ref["flags"] == 0
            assert ref["K"] == 3 * 20 * 32
            for loading in (0.0, 0.5):
                W, delta, flags, _ = AR.weights(np.eye(nrx), a, loading)
                assert flags == 0 and delta == loading
                np.testing.assert_allclose(W, AR.conventional(a), rtol=1e-13, atol=1e-15)
        nus = [0.1, -0.3]
        np.testing.assert_allclose(AR.conventional(steering_vectors(nrx, nus)), steering_weights(nrx, nus), atol=1e-7)


def test_fallback_on_a_rank_deficient_covariance():
    """n_rx 4 with two channels identical and no loading: a pivot at the rounding level, the flag and
    the conventional weights; with loading the same input solves."""
    spec = np.array(AR.noise_scene(32, 4)[:1])
    spec[:, 2] = spec[:, 1]
    a = AR.case_constraints(4, 3, seed=5)[1]
    ref = AR.adapt_ref(spec, a, 0.0)
    assert ref["flags"] == AR.FALLBACK and ref["delta"] == 0.0
    np.testing.assert_array_equal(ref["W"], AR.conventional(a))
    ok = AR.adapt_ref(spec, a, 1e-2)
    assert ok["flags"] == 0 and np.abs(np.einsum("bk,bk->b", ok["W"], a.astype(np.complex128)) - 1).max() <= 1e-12
    W, _, flags, _ = AR.weights(-np.eye(3), np.ones((1, 3)), 0.0)      # not positive: the first pivot
    assert flags == AR.FALLBACK and np.allclose(W, 1 / 3)


def test_jammer_scene_margins():
    """adapt_ref.jammer_scene as built (seed 7: unit noise, jammer 40 dB at nu -0.3, target amplitude 1
    = 13.7 dB per channel after the Doppler sum at cell (20, 5), nu 0.1), through beams_ref and the
    oracle's 2-D OS-CFAR.  Measured on the CPU: the conventional beam holds the cell at 0.39 of its
    threshold (missed), the adaptive one (loading 1e-2) at 2.8 times (detected), and the adaptive
    response at the jammer is 58 dB below the conventional one; seeds 8, 9, 10 give 0.13 .. 0.23,
    2.6 .. 3.1 and 53 .. 57 dB.  Asserted with room: <= 0.7, >= 1.5, >= 30 dB."""
    spec = AR.jammer_scene()
    a = steering_vectors(AR.JAM_NRX, [AR.JAM_NU_T])
    wc = steering_weights(AR.JAM_NRX, [AR.JAM_NU_T])
    ref = AR.adapt_ref(spec, a, 1e-2)
    r, d = AR.JAM_CELL
    ratio = {}
    for kind, w in (("conventional", wc), ("adaptive", ref["W"])):
        m = beams_ref(spec, w)[0][0, 0].astype(np.float32)
        det, thr = O.cfar_os2d(m, O.Cfar2D())
        ratio[kind] = float(m[r, d] / thr[r, d])
        assert bool(det[r, d]) == (kind == "adaptive"), (kind, ratio[kind])
    aj = steering_vectors(AR.JAM_NRX, [AR.JAM_NU_J])[0].astype(np.complex128)
    null_db = 20 * np.log10(abs(ref["W"][0] @ aj) / abs(wc[0].astype(np.complex128) @ aj))
    print(f"\ncell / threshold: {ratio}; adaptive over conventional at the jammer: {null_db:.1f} dB")
    assert ratio["conventional"] <= 0.7 and ratio["adaptive"] >= 1.5 and null_db <= -30.0
    assert AR.w_bound(ref, AR.gamma(1, AR.JAM_NR, AR.JAM_NC)) <= AR.W_BOUND_MAX


@pytest.mark.parametrize("nd", AR.DOPPLERS)
def test_gpu_inputs_are_within_the_bound(nd):
    """Every input of tests/test_gpu_adapt.py's matrix, on the reference alone: no fallback, loading
    >= 1e-3, and the perturbation bound on W under W_BOUND_MAX (a case over it would fail there as a
    bad input)."""
    worst = 0.0
    for nrx in AR.RXS:
        spec = AR.noise_scene(nd, nrx)
        assert np.all(np.abs(spec).reshape(3, nrx, -1).min(axis=2) > 0)          # noise in every channel
        for mti in AR.MTIS:
            nf, (r0, rows, loading) = AR.matrix_case(nd, nrx, mti)
            assert loading >= 1e-3
            for a in AR.case_constraints(nrx, 3, seed=1000 * nd + 10 * nrx + mti):
                ref = AR.adapt_ref(spec[:nf], a, float(np.float32(loading)), mti, r0, rows)
                assert ref["flags"] == 0
                worst = max(worst, AR.w_bound(ref, AR.gamma(nf, rows, nd)))
    print(f"\nn_doppler {nd}: the largest bound on W is {worst:.3g} relative")
    assert worst <= AR.W_BOUND_MAX


@pytest.mark.parametrize("nd", AR.DOPPLERS)
def test_full_scale_inputs_are_within_the_bound(nd):
    """The full-scale cases of tests/test_gpu_adapt.py on the reference alone: white noise gives a
    well-conditioned covariance, so no fallback, and the bound on W far under W_BOUND_MAX."""
    for nrx in AR.FS_RXS:
        for mti in AR.MTIS:
            spec, a = AR.full_scale_case(nd, nrx, mti)
            ref = AR.adapt_ref(spec, a, float(np.float32(AR.FS_LOADING)), mti)
            wb = AR.w_bound(ref, AR.gamma(AR.FS_NF, AR.NR, nd))
            print(f"\nfull scale {AR.NR}x{nd} rx{nrx} mti{mti}: cond(Rl) {np.linalg.cond(ref['Rl']):.3g}, "
                  f"bound on W {wb:.3g} relative")
            assert ref["flags"] == 0 and ref["K"] == AR.FS_NF * AR.NR * nd
            assert np.linalg.cond(ref["Rl"]) < 10.0 and wb <= AR.W_BOUND_MAX


def test_chain_length():
    assert AR.chain_length(1, 1, 32) == (64, 1)            # half a step
    assert AR.chain_length(1, 3, 32) == (64, 2) and AR.chain_length(3, 3, 32) == (64, 6)
    assert AR.chain_length(3, 64, 1024) == (128, 2048)     # 3072 steps over 2048 units
    assert AR.chain_length(8, 512, 4096 // 4) == (64 * 32, 2048)


def test_cli_arguments(tmp_path, capsys):
    for bad in (["--adaptive", "0.01"], ["--beams", "4", "--adaptive", "-1"], ["--beams", "4", "--adaptive", "nan"]):
        with pytest.raises(SystemExit):
            cli.main([str(tmp_path / "x.npy")] + bad)
        assert "--adaptive" in capsys.readouterr().err
