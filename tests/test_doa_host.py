"""The angle resolver without a GPU: the C-ABI's layout, exports and argument checks (they come before any
device access), the steering builders, and on tests/doa_ref.py alone: the physics (what the phase-step
estimator reads where two targets share a cell, and what the resolver reads), how many sources of each GPU
case the parabola's conditioning leaves out, and what a kernel with each modelled defect would change."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import fmcw_oracle as O
from fmcw import _lib as L
from fmcw import DOA_DTYPE, AngleResolver, calibrated, line_steering, planar_steering, synth
import bearings_ref as B
import doa_ref as D
import mimo_ref as M

NEW_SYMBOLS = ("fmcw_doa_config_default", "fmcw_doa_create", "fmcw_doa_destroy", "fmcw_doa_set_steering",
               "fmcw_doa_set_steering_dev", "fmcw_doa_enqueue", "fmcw_doa_set_grid_for_test")
NAMES = ["n_ch", "n_grid", "k_max", "relax_passes", "min_rel", "refine", "max_records", "device_id"]


def default_cfg(lib):
    cfg = L.FmcwDoaConfig()
    lib.fmcw_doa_config_default(C.byref(cfg))
    return cfg


# ---- ABI -------------------------------------------------------------------------------------------
def test_layout_and_defaults(lib_built):
    assert C.sizeof(L.FmcwDoa) == 96 == DOA_DTYPE.itemsize and C.sizeof(L.FmcwDoaSrc) == 16
    assert C.sizeof(L.FmcwDoaConfig) == 32
    assert [f[0] for f in L.FmcwDoaConfig._fields_] == NAMES
    assert [getattr(L.FmcwDoaConfig, n).offset for n in NAMES] == [0, 4, 8, 12, 16, 20, 24, 28]
    assert [DOA_DTYPE.fields[k][1] for k in ("frame", "range", "doppler", "flags", "n_src", "total", "residual",
                                             "reserved", "src")] == [0, 4, 6, 8, 12, 16, 20, 24, 32]
    assert [getattr(L.FmcwDoa, k).offset for k in ("flags", "n_src", "total", "residual", "reserved", "src")] == [8, 12, 16, 20, 24, 32]
    src = L.HEADER_PATH.read_text()
    body = src[src.index("typedef struct fmcw_doa_config {"):src.index("} fmcw_doa_config;")]
    at = [body.index(n + ";") for n in NAMES]
    assert at == sorted(at)
    cfg = default_cfg(lib_built)
    assert (cfg.n_ch, cfg.n_grid, cfg.k_max, cfg.relax_passes, cfg.refine) == (16, 256, 2, 2, 1)
    assert (cfg.min_rel, cfg.max_records, cfg.device_id) == (np.float32(0.02), 1 << 20, 0)
    assert (L.DOA_NO_SNAPSHOT, L.DOA_ONE_CH, L.DOA_STATUS_WORDS, L.DOA_MAX_SRC) == (1, 2, 2, 4)
    for text in ("#define FMCW_DOA_NO_SNAPSHOT 1u", "#define FMCW_DOA_ONE_CH 2u", "#define FMCW_DOA_STATUS_WORDS 2",
                 "#define FMCW_DOA_MAX_SRC 4", "Still 8 with the angle resolver"):
        assert text in src, text
    assert lib_built.fmcw_abi_version() == 8


def test_new_symbols_exported(lib_built):
    out = subprocess.run(["nm", "-D", "--defined-only", str(L.LIB_PATH)], capture_output=True, text=True,
                         check=True).stdout
    src = L.HEADER_PATH.read_text()
    for name in NEW_SYMBOLS:
        assert f" T {name}\n" in out, name
        assert name in L.SIGNATURES and f"{name}(" in src


# (fields to set, the whole message), in the order fmcw_doa_create checks them
BAD_FIELDS = [
    (dict(n_ch=0), b"n_ch=0: must be in [1, 64]"),
    (dict(n_ch=65), b"n_ch=65: must be in [1, 64]"),
    (dict(n_grid=0), b"n_grid=0: must be a multiple of 64 in [64, 1024]"),
    (dict(n_grid=96), b"n_grid=96: must be a multiple of 64 in [64, 1024]"),
    (dict(n_grid=1088), b"n_grid=1088: must be a multiple of 64 in [64, 1024]"),
    (dict(k_max=0), b"k_max=0: must be in [1, 4]"),
    (dict(k_max=5), b"k_max=5: must be in [1, 4]"),
    (dict(relax_passes=4), b"relax_passes=4: must be in [0, 3]"),
    (dict(min_rel=-0.1), b"min_rel -0.1: must be in [0, 1)"),
    (dict(min_rel=1.0), b"min_rel 1: must be in [0, 1)"),
    (dict(min_rel=float("nan")), b"min_rel nan: must be in [0, 1)"),
    (dict(refine=2), b"refine=2: must be 0 or 1"),
    (dict(max_records=0), b"max_records 0 (1..2^31-1)"),
    (dict(max_records=1 << 31), b"max_records 2147483648 (1..2^31-1)"),
    (dict(device_id=-1), b"device_id -1 (0..63)"),
    (dict(device_id=64), b"device_id 64 (0..63)"),
]


@pytest.mark.parametrize("fields,msg", BAD_FIELDS, ids=[m.decode().split(":")[0].split(" (")[0] + f"#{i}"
                                                        for i, (_, m) in enumerate(BAD_FIELDS)])
def test_create_rejects_bad_fields(lib_built, fields, msg):
    """FMCW_EINVAL with the field's name, before any device access; the handle stays null."""
    cfg = default_cfg(lib_built)
    for k, v in fields.items():
        setattr(cfg, k, v)
    h = C.c_void_p(1)
    assert lib_built.fmcw_doa_create(C.byref(cfg), C.byref(h)) == L.FMCW_EINVAL
    assert lib_built.fmcw_last_error() == msg
    assert not h.value


def test_null_arguments_and_device(lib_built):
    assert lib_built.fmcw_doa_create(None, None) == L.FMCW_EINVAL
    assert lib_built.fmcw_doa_destroy(None) == L.FMCW_OK
    assert lib_built.fmcw_doa_set_grid_for_test(None, 1) == L.FMCW_EINVAL
    assert lib_built.fmcw_last_error() == b"null angle resolver"
    assert lib_built.fmcw_doa_set_steering(None, None, None) == L.FMCW_EINVAL
    assert lib_built.fmcw_doa_set_steering_dev(None, None, None) == L.FMCW_EINVAL
    assert lib_built.fmcw_doa_enqueue(None, None, None, 0, 1, None, None, None, None, None) == L.FMCW_EINVAL
    lib_built.fmcw_doa_config_default(None)
    for fields in (dict(), dict(n_ch=64, n_grid=1024, k_max=4, relax_passes=3), dict(n_ch=1, n_grid=64, min_rel=0.0)):
        cfg = default_cfg(lib_built)
        for k, v in fields.items():
            setattr(cfg, k, v)
        h = C.c_void_p(1)
        rc = lib_built.fmcw_doa_create(C.byref(cfg), C.byref(h))
        if L.device_count() > 0:
            assert rc == L.FMCW_OK and h.value, lib_built.fmcw_last_error()
            zero_row = np.ones((cfg.n_grid, cfg.n_ch), np.complex64)     # the zero-norm row is named
            zero_row[5] = 0
            assert lib_built.fmcw_doa_set_steering(h, zero_row.ctypes.data, None) == L.FMCW_EINVAL
            assert lib_built.fmcw_last_error().startswith(b"steering_host: row 5 has norm 0")
            assert lib_built.fmcw_doa_destroy(h) == L.FMCW_OK
        else:
            assert rc == L.FMCW_ENODEV and not h.value
            assert lib_built.fmcw_last_error() == b"no HIP device"


def test_python_builders(lib_built):
    a, st = line_steering(16, 0.5, 256)
    ref, nu = D.line_table(16, 256)
    assert a.dtype == np.complex64 and np.array_equal(a, ref) and np.allclose(0.5 * st, nu)
    pos = np.stack([np.arange(4) * 0.5, np.zeros(4)], axis=1)
    u = np.stack([st, np.zeros_like(st)], axis=1)
    assert np.allclose(planar_steering(pos, u), a[:, :4], atol=1e-6)
    gains = np.exp(2j * np.pi * np.arange(16) / 7)
    assert np.allclose(calibrated(a, gains), a * gains[None, :], atol=1e-6)
    with pytest.raises(ValueError):
        calibrated(a, gains[:3])
    with pytest.raises(ValueError):
        planar_steering(pos, np.zeros((4, 3)))
    with pytest.raises(ValueError):
        AngleResolver(8, a)
    with pytest.raises(L.FmcwError, match="k_max=9"):
        AngleResolver(16, a, k_max=9)


def test_two_in_cell_frames():
    a = synth.two_in_cell_frames(2, 64, 64, 4, 2, cell=(9, 3), rx_phase=(0.1, -0.2), seed=3)
    assert a.dtype == np.complex64 and a.shape == (2, 4, 64, 64)
    for t in range(2):                                                   # one transmitter's chirps: [chirp][sample]
        mag = np.abs(np.fft.fft2(a[0, 0, t::2].astype(np.complex128)))
        assert np.unravel_index(mag.argmax(), mag.shape) == (3, 9)
    with pytest.raises(ValueError):
        synth.two_in_cell_frames(1, 64, 64, 4, 3)
    with pytest.raises(ValueError):
        synth.two_in_cell_frames(1, 64, 64, 4, 2, rx_phase=(0.1,), amps=(1.0, 2.0))


# ---- the physics, on the reference alone -------------------------------------------------------------
def chain_snapshot(n_tx, n_rx):
    """two_in_cell_frames -> the oracle's range stage -> mimo_ref -> bearings_ref at the targets' cell."""
    cube = synth.two_in_cell_frames(1, D.CHAIN_NS, D.CHAIN_NC, n_rx, n_tx, cell=D.CHAIN_CELL, rx_phase=D.CHAIN_NUS,
                                    seed=D.CHAIN_SEED)
    spec = O.range_ct(cube[0])[None]
    rec = np.zeros(1, np.dtype([("frame", "<u4"), ("range", "<u2"), ("doppler", "<u2")]))
    rec["range"], rec["doppler"] = D.CHAIN_CELL
    out, sn, _ = B.bearings_ref(M.mimo_ref(spec, n_tx, "dft"), rec)
    return out, sn.astype(np.complex64)


def nu_of(pos, n_grid):
    return 0.5 * (-1.0 + 2.0 * np.asarray(pos) / n_grid)


@pytest.mark.parametrize("n_tx,n_rx", D.CHAIN_ARRAYS)
def test_two_targets_in_one_cell(n_tx, n_rx):
    """16 virtual elements, nu 0.10 and 0.22, amplitudes 1 and 0.7, a 256-point grid (a step of 1 / 256 in
    nu).  Measured, both arrays alike: the phase step reads nu 0.1380 at coherence 0.978, 9.7 steps from
    the nearer target; the scan with cancellation reads 0.0984 / 0.2203, with two RELAX passes 0.1001 /
    0.2199 (0.04 steps)."""
    bear, sn = chain_snapshot(n_tx, n_rx)
    steering, _ = D.line_table(n_tx * n_rx, D.CHAIN_GRID)
    step = 1.0 / D.CHAIN_GRID
    res = D.resolve_list(sn, steering, k_max=2, relax_passes=2)[0]
    est = np.sort(nu_of(res["pos"], D.CHAIN_GRID))
    print(f"\n{n_tx} TX x {n_rx} RX: phase step {bear['nu'][0]:.4f} (coherence {bear['coherence'][0]:.3f}), resolver {est}")
    assert res["n_src"] == 2 and np.all(np.abs(est - np.sort(D.CHAIN_NUS)) <= 0.5 * step)
    assert min(abs(bear["nu"][0] - nu) for nu in D.CHAIN_NUS) > 4 * step


def test_three_sources_on_64_elements():
    """64 elements, a 1024-point grid (a step of 1 / 1024 in nu), sources at nu -0.2, 0.10, 0.13 with
    amplitudes 1, 0.8, 0.6.  Measured over 40 noise draws: the phase step is 141 steps or more from every
    source; three stages alone are up to 1.9 steps off, with two RELAX passes 0.065 steps at most."""
    nus = (-0.2, 0.10, 0.13)
    steering, _ = D.line_table(64, 1024)
    sn = D.planted(40, 64, nus, (1.0, 0.8, 0.6), 0.01, 7)
    res = D.resolve_list(sn, steering, k_max=3, relax_passes=2)
    est = np.sort([nu_of(r["pos"], 1024) for r in res], axis=1)
    worst = np.abs(est - np.sort(nus)).max() * 1024
    off = np.abs(D.phase_step_nu(sn)[:, None] - np.array(nus)).min() * 1024
    print(f"\n64 elements: resolver at most {worst:.3f} grid steps off, phase step at least {off:.1f}")
    assert all(r["n_src"] == 3 for r in res) and worst <= 0.5 and off > 4


def test_planar_array_without_refine():
    """A 4 x 4 half-wavelength planar array, a 16 x 16 grid of direction cosines in row-major order (256 rows,
    neighbouring rows are not neighbouring angles: refine off): two sources on grid directions are found at
    their rows."""
    ix, iy = np.meshgrid(np.arange(4), np.arange(4), indexing="ij")
    pos = 0.5 * np.stack([ix.ravel(), iy.ravel()], axis=1)
    u = -1.0 + 2.0 * np.arange(16) / 16
    dirs = np.stack([np.repeat(u, 16), np.tile(u, 16)], axis=1)
    steering = planar_steering(pos, dirs)
    rows = (5 * 16 + 11, 12 * 16 + 3)
    rng = np.random.default_rng(2)
    sn = 1000.0 * (steering[rows[0]] + 0.7j * steering[rows[1]]) + 10.0 * (rng.standard_normal(16) + 1j * rng.standard_normal(16))
    res = D.resolve(sn.astype(np.complex64), D.Table(steering), k_max=2, relax_passes=2, refine=False)
    assert res["grid"] == list(rows) and res["pos"] == [float(r) for r in rows]
    assert abs(abs(res["amp"][0]) - 1000) < 20 and abs(abs(res["amp"][1]) - 700) < 20


def test_calibration_table():
    """Per-channel phase errors of up to +-0.4 cycles: with the calibrated table the two sources are within
    half a grid step, with the ideal table at least one of them is off by more than four."""
    nus, n_grid = (0.10, 0.22), 256
    steering, _ = D.line_table(16, n_grid)
    gains = np.exp(2j * np.pi * np.random.default_rng(11).uniform(-0.4, 0.4, 16))
    sn = (D.planted(20, 16, nus, (1.0, 0.7), 0.01, 5).astype(np.complex128) * gains[None, :]).astype(np.complex64)
    good = D.resolve_list(sn, calibrated(steering, gains), k_max=2, relax_passes=2)
    bad = D.resolve_list(sn, steering, k_max=2, relax_passes=2)
    err = lambda res: np.array([np.abs(np.sort(nu_of((r["pos"] + [0.0, 0.0])[:2], n_grid)) - np.sort(nus)).max() for r in res]) * n_grid
    print(f"\ncalibrated: at most {err(good).max():.3f} steps off; ideal table: at least {err(bad).min():.1f}")
    assert err(good).max() <= 0.5 and err(bad).min() > 4


# ---- the comparison's own limits ---------------------------------------------------------------------
@pytest.mark.parametrize("case", D.GPU_CASES, ids=D.case_id)
def test_gpu_cases_keep_the_parabola_conditioned(case):
    """On the reference alone, before any GPU value: at most 5 % of a GPU case's sources are left to the
    skip for pos (measured: 0 in every case of the matrix)."""
    snaps, steering, cfg = D.gpu_case(case)
    share = D.skipped_share(snaps[:60], steering, **cfg)
    print(f"\n{D.case_id(case)}: {100 * share:.1f} % of the sources skipped for pos")
    assert share <= D.SKIP_SHARE


def test_forced_picks_are_checked():
    """assert_doa_match's core: the reference's own output passes as the GPU's; a pick one beam away, a
    wrong source count and an amplitude off by 1e-4 do not."""
    steering, _ = D.line_table(16, 128)
    tab = D.Table(steering)
    s = D.planted(1, 16, (0.10, 0.22), (1.0, 0.7), 0.01, 3)[0]
    own = D.resolve(s, tab, k_max=2, relax_passes=1)
    again = D.resolve(s, tab, k_max=2, relax_passes=1, picks=own["picked"], n_src=2)
    assert again["why"] is None and again["amp"] == own["amp"] and len(own["picked"]) == 2
    moved = [list(own["picked"][0]), [own["picked"][1][0] + 9, own["picked"][1][1]]]
    assert "pick" in D.resolve(s, tab, k_max=2, relax_passes=1, picks=moved, n_src=2)["why"]
    assert "goes on" in D.resolve(s, tab, k_max=2, relax_passes=1, picks=[own["picked"][0][:1]] * 2, n_src=1)["why"]
    assert own["e_amp"][0] < 1e-4 * abs(own["amp"][0])


# ---- what the comparison can tell apart ----------------------------------------------------------------
DEFECT_SHARE = 0.5     # a defect must change more than half of the scene's records


def changed(ref, other, n_grid):
    """Whether a record's output differs beyond anything rounding does: another source count or grid point,
    pos by more than 0.01, an amplitude by more than 1e-3 of the strongest."""
    if ref["n_src"] != other["n_src"] or ref["grid"] != other["grid"]:
        return True
    top = max(abs(a) for a in ref["amp"])
    return any(abs(p - q) > 0.01 for p, q in zip(ref["pos"], other["pos"])) or \
        any(abs(a - b) > 1e-3 * top for a, b in zip(ref["amp"], other["amp"]))


@pytest.mark.parametrize("defect", D.DEFECTS)
def test_defect_catalogue(defect):
    """Each modelled defect changes more than half of the records of the planted 16-element scene of the GPU
    matrix (for the tie rule: of that scene on a table whose second half repeats its first, where every
    maximum is an exact tie)."""
    case = next(c for c in D.GPU_CASES if c["kind"] == "planted" and c["n_ch"] == 16)
    snaps, steering, cfg = D.gpu_case(case)
    snaps = snaps[:40]
    if defect == "highest_tie":
        steering = np.concatenate([steering[:64], steering[:64]])
    ref = D.resolve_list(snaps, steering, **cfg)
    other = D.resolve_list(snaps, steering, defect=defect, **cfg)
    share = float(np.mean([changed(a, b, len(steering)) for a, b in zip(ref, other)]))
    print(f"\n{defect}: changes {100 * share:.0f} % of the records")
    assert share > DEFECT_SHARE
