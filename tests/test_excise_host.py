"""The interference exciser without a GPU: the C-ABI's layout, exports and argument checks (they come
before any device access), the specification (tests/excise_ref.py) against its independent brute force,
hand cases with known answers, synth.interference_bursts, the CLI's arguments, and the end-to-end claim
under the project's oracle: a weak target lost under the bursts is found again on the repaired cube."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import excise_ref as R
import fmcw_oracle as O
from fmcw import _lib as L
from fmcw import InterferenceExciser, cli, synth

NEW_SYMBOLS = ("fmcw_excise_config_default", "fmcw_excise_create", "fmcw_excise_destroy", "fmcw_excise_enqueue",
               "fmcw_excise_set_grid_for_test")
DTYPES = ("f32", "f16", "i16")


def default_cfg(lib):
    cfg = L.FmcwExciseConfig()
    lib.fmcw_excise_config_default(C.byref(cfg))
    return cfg


def test_layout_and_defaults(lib_built):
    assert C.sizeof(L.FmcwExciseConfig) == 48
    names = ["n_range", "n_doppler", "n_rx", "in_dtype", "mode", "guard", "rank_pct", "alpha", "max_frames",
             "device_id", "reserved"]
    assert [f[0] for f in L.FmcwExciseConfig._fields_] == names
    for i, name in enumerate(names):
        assert getattr(L.FmcwExciseConfig, name).offset == 4 * i
    assert L.FmcwExciseConfig.reserved.size == 8
    src = L.HEADER_PATH.read_text()
    body = src[src.index("typedef struct fmcw_excise_config {"):src.index("} fmcw_excise_config;")]
    decl = [n + ("[2];" if n == "reserved" else ";") for n in names]
    assert all(d in body for d in decl)                                   # every field, in this order
    assert sorted(decl, key=body.index) == decl
    assert "float alpha;" in body and "int32_t mode;" in body and "int32_t in_dtype;" in body
    assert "int32_t device_id;" in body and "uint32_t n_rx;" in body
    cfg = default_cfg(lib_built)
    assert (cfg.n_range, cfg.n_doppler, cfg.n_rx, cfg.in_dtype, cfg.mode) == (1024, 128, 1, L.IN_F32, L.EXCISE_ZERO)
    assert (cfg.guard, cfg.rank_pct, cfg.alpha, cfg.max_frames, cfg.device_id) == (4, 50, 16.0, 1, 0)
    assert tuple(cfg.reserved) == (0, 0)
    assert (L.EXCISE_ZERO, L.EXCISE_INTERP, L.EXCISE_STATUS_WORDS) == (0, 1, 4)
    assert "FMCW_EXCISE_ZERO = 0" in src and "FMCW_EXCISE_INTERP = 1" in src
    assert "#define FMCW_EXCISE_STATUS_WORDS 4" in src
    assert lib_built.fmcw_abi_version() == 8 and "Still 8 with the interference exciser" in src


def test_new_symbols_exported(lib_built):
    out = subprocess.run(["nm", "-D", "--defined-only", str(L.LIB_PATH)], capture_output=True, text=True,
                         check=True).stdout
    src = L.HEADER_PATH.read_text()
    for name in NEW_SYMBOLS:
        assert f" T {name}\n" in out, name
        assert name in L.SIGNATURES and f"{name}(" in src


def _set(cfg, field, value):
    if field == "reserved0":
        cfg.reserved[0] = value
    elif field == "reserved1":
        cfg.reserved[1] = value
    else:
        setattr(cfg, field, value)


@pytest.mark.parametrize("fields,msg", [
    ({"n_range": 1000}, b"n_range"), ({"n_range": 32}, b"n_range"), ({"n_range": 16384}, b"n_range"),
    ({"n_range": 0}, b"n_range"),
    ({"n_doppler": 0}, b"n_doppler"), ({"n_doppler": 1025}, b"n_doppler"),
    ({"n_rx": 0}, b"n_rx"), ({"n_rx": 65}, b"n_rx"),
    ({"in_dtype": 3}, b"in_dtype"), ({"in_dtype": -1}, b"in_dtype"),
    ({"mode": 2}, b"mode"), ({"mode": -1}, b"mode"),
    ({"guard": 33}, b"guard"), ({"guard": 0xFFFFFFFF}, b"guard"),
    ({"rank_pct": 0}, b"rank_pct"), ({"rank_pct": 100}, b"rank_pct"),
    ({"alpha": 0.5}, b"alpha"), ({"alpha": -16.0}, b"alpha"), ({"alpha": float("nan")}, b"alpha"),
    ({"alpha": float("inf")}, b"alpha"),
    ({"max_frames": 0}, b"max_frames"), ({"max_frames": 1 << 15}, b"max_frames"),   # 2^15 x 2^17 samples = 2^32
    ({"n_range": 8192, "n_doppler": 1024, "n_rx": 64, "max_frames": 8}, b"max_frames"),
    ({"reserved0": 1}, b"reserved"), ({"reserved1": 7}, b"reserved"),
    ({"device_id": -1}, b"device_id"), ({"device_id": 64}, b"device_id"),
])
def test_create_rejects_bad_fields(lib_built, fields, msg):
    cfg = default_cfg(lib_built)
    for k, v in fields.items():
        _set(cfg, k, v)
    h = C.c_void_p(1)
    rc = lib_built.fmcw_excise_create(C.byref(cfg), C.byref(h))
    assert rc == L.FMCW_EINVAL
    assert msg in lib_built.fmcw_last_error(), lib_built.fmcw_last_error()
    assert not h.value


def test_create_accepts_the_edges_of_the_ranges(lib_built):
    """The largest product below 2^32, a chirp count that is no power of two, alpha 1, guard 32: past
    validation, so the answer is the device's (FMCW_ENODEV without one)."""
    for fields in ({"max_frames": (1 << 15) - 1}, {"n_doppler": 3, "n_rx": 64, "guard": 32, "alpha": 1.0, "rank_pct": 99},
                   {"n_range": 64, "n_doppler": 1, "in_dtype": L.IN_I16, "mode": L.EXCISE_INTERP, "guard": 0, "rank_pct": 1}):
        cfg = default_cfg(lib_built)
        for k, v in fields.items():
            _set(cfg, k, v)
        h = C.c_void_p(1)
        rc = lib_built.fmcw_excise_create(C.byref(cfg), C.byref(h))
        if L.device_count() > 0:
            assert rc == L.FMCW_OK and lib_built.fmcw_excise_destroy(h) == L.FMCW_OK
        else:
            assert rc == L.FMCW_ENODEV and not h.value


def test_null_arguments(lib_built):
    assert lib_built.fmcw_excise_create(None, None) == L.FMCW_EINVAL
    assert lib_built.fmcw_excise_destroy(None) == L.FMCW_OK
    assert lib_built.fmcw_excise_set_grid_for_test(None, 1) == L.FMCW_EINVAL
    assert lib_built.fmcw_last_error() == b"null exciser"
    assert lib_built.fmcw_excise_enqueue(None, None, 1, None, None, None, None, None) == L.FMCW_EINVAL
    assert lib_built.fmcw_last_error() == b"null exciser"
    lib_built.fmcw_excise_config_default(None)


def test_create_without_device_fails_cleanly(lib_built):
    cfg = default_cfg(lib_built)
    h = C.c_void_p(1)
    rc = lib_built.fmcw_excise_create(C.byref(cfg), C.byref(h))
    if L.device_count() > 0:      # a valid configuration: the GPU tests take it from here
        assert rc == L.FMCW_OK and h.value
        assert lib_built.fmcw_excise_destroy(h) == L.FMCW_OK
    else:
        assert rc == L.FMCW_ENODEV and not h.value
        assert lib_built.fmcw_last_error() == b"no HIP device"


def test_python_class_and_constants(lib_built):
    assert InterferenceExciser.__init__.__defaults__ == (1024, 128, 1, "f32", "zero", 4, 50, 16.0, 1, 0)
    assert InterferenceExciser._SYM == "fmcw_excise"
    for name in ("enqueue", "repair", "set_grid_for_test", "close", "__enter__", "__exit__"):
        assert callable(getattr(InterferenceExciser, name))
    with pytest.raises(KeyError):
        InterferenceExciser(64, 32, mode="blank")
    with pytest.raises(KeyError):
        InterferenceExciser(64, 32, in_dtype="f64")
    with pytest.raises(L.FmcwError, match="guard"):
        InterferenceExciser(64, 32, guard=33)
    with pytest.raises(L.FmcwError, match="alpha"):
        InterferenceExciser(64, 32, alpha=0.99)


# ---- the specification against the definitions ----------------------------------------------------
def noise_line(rng, ns, dtype, scale=1.0):
    z = (rng.standard_normal(ns) + 1j * rng.standard_normal(ns)) * scale
    if dtype == "f32":
        return z.astype(np.complex64)
    iq = np.stack([z.real, z.imag], axis=-1)
    return np.rint(iq * 200).astype(np.int16) if dtype == "i16" else (iq / 8).astype(np.float16)


def add_burst(line, at, length, amp):
    line = line.copy()
    n = np.arange(length)
    b = amp * np.exp(2j * np.pi * (0.11 * n + 0.003 * n * n))
    if line.dtype == np.complex64:
        line[at:at + length] += b.astype(np.complex64)
    elif line.dtype == np.int16:
        line[at:at + length] = np.clip(line[at:at + length] + np.rint(np.stack([b.real, b.imag], -1) * 200), -32768, 32767)
    else:
        line[at:at + length] = (line[at:at + length].astype(np.float32) + np.stack([b.real, b.imag], -1) / 8).astype(np.float16)
    return line


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", [R.ZERO, R.INTERP])
def test_reference_against_the_brute_force(dtype, mode):
    """Random lines of 64 and 256 samples with 0 to 3 bursts, several guards, ranks and alphas: the
    float32 restatement gives the brute force's bytes, mask, count and status words."""
    rng = np.random.default_rng(11)
    seen = 0
    for trial in range(24):
        ns = (64, 256)[trial % 2]
        line = noise_line(rng, ns, dtype)
        for _ in range(trial % 4):
            length = int(rng.integers(1, 20))
            line = add_burst(line, int(rng.integers(0, ns - length + 1)), length, 30.0)
        guard = (0, 1, 4, 32)[trial % 4 if trial < 20 else 3]
        rank_pct, alpha = ((50, 16.0), (1, 64.0), (99, 1.0), (50, 1.0))[(trial // 4) % 4]
        got = R.excise(line[None], mode, guard, rank_pct, alpha)
        want = R.brute_force(line, mode, guard, rank_pct, alpha)
        assert same(got[0][0], want[0]), (trial, guard, rank_pct, alpha)
        assert np.array_equal(got[1][0], want[1]) and got[2][0] == want[2]
        assert got[3].tolist() == want[3].tolist()
        assert same(got[0][0][~want[1]], line[~want[1]])          # outside every run: the input's bits
        seen += int(want[2])
    assert seen > 500


def test_exact_order_statistic_on_ties():
    """An int16 line whose powers tie around the rank: 40 samples of power 25 (3, 4), (5, 0), (0, -5),
    (-4, 3), 24 of power 2.  k = 32 falls inside the tied block: m = 25, T = 2 x 25 = 50; with rank_pct
    37 (k = 23) m = 2 and T = 4: the 40 tied samples are all flagged, none of the small ones."""
    line = np.zeros((64, 2), np.int16)
    line[:] = (1, -1)
    tied = [(3, 4), (5, 0), (0, -5), (-4, 3)]
    for i, n in enumerate(range(0, 64, 8)):
        for j in range(5):
            line[n + j] = tied[(i + j) % 4]
    p = R.power(line)
    assert sorted(set(p.tolist())) == [2.0, 25.0] and (p == 25).sum() == 40
    assert R.level(p, 50) == 25.0 and R.level(p, 37) == 2.0 and R.level(p, 38) == 25.0
    out, g, counts, st = R.excise(line[None], R.ZERO, 0, 50, 2.0)
    assert st.tolist() == [0, 0, 0, 0] and same(out[0], line)
    out, g, counts, st = R.excise(line[None], R.ZERO, 0, 37, 2.0)
    assert st.tolist() == [40, 1, 40, 1] and np.array_equal(g[0], p == 25)
    assert np.all(out[0][p == 25] == 0) and same(out[0][p == 2], line[p == 2])
    for a, b in zip(R.excise(line[None], R.INTERP, 0, 37, 2.0), (None, g, counts, st)):
        assert b is None or np.array_equal(a, b)


def quiet(ns, dtype="f32"):
    """A line of constant power 2 with a slowly turning phase, so every neighbour differs."""
    if dtype == "i16":
        out = np.zeros((ns, 2), np.int16)
        out[:, 0] = 10 + np.arange(ns) % 7
        out[:, 1] = -10 + np.arange(ns) % 5
        return out
    n = np.arange(ns)
    return (np.sqrt(2.0) * np.exp(2j * np.pi * n / 37.0)).astype(np.complex64)


def hot(line, where, amp=1000.0):
    line = line.copy()
    for n in where:
        line[n] = amp if line.dtype == np.complex64 else (int(amp), 0)
    return line


def run_of(g):
    return R.runs_of(g)


def test_bursts_at_the_ends_of_the_line():
    """Flags at sample 0 and at Ns - 1, guard 4: runs [0, 4] and [Ns - 5, Ns - 1]; ZERO blanks them,
    INTERP holds the one neighbour each has."""
    ns = 64
    line = hot(quiet(ns), [0, ns - 1])
    out, g, counts, st = R.excise(line[None], R.ZERO, 4)
    assert run_of(g[0]) == [(0, 4), (ns - 5, ns - 1)] and counts.tolist() == [10] and st.tolist() == [10, 1, 2, 0]
    assert np.all(out[0][g[0]] == 0) and same(out[0][~g[0]], line[~g[0]])
    out, g2, _, st2 = R.excise(line[None], R.INTERP, 4)
    assert np.array_equal(g, g2) and st2.tolist() == st.tolist()
    assert np.all(out[0][:5] == line[5]) and np.all(out[0][ns - 5:] == line[ns - 6])
    assert same(out[0][~g[0]], line[~g[0]])


def test_two_bursts_merge_at_twice_the_guard():
    """Two flags with 2 guard clean samples between them dilate into one run (the guards meet); with
    2 guard + 1 between them into two runs, one clean sample apart."""
    ns, guard = 64, 4
    line = hot(quiet(ns), [20, 21 + 2 * guard])
    _, g, counts, st = R.excise(line[None], R.ZERO, guard)
    assert run_of(g[0]) == [(16, 33)] and st.tolist() == [18, 1, 2, 0]
    line = hot(quiet(ns), [20, 22 + 2 * guard])
    out, g, counts, st = R.excise(line[None], R.INTERP, guard)
    assert run_of(g[0]) == [(16, 24), (26, 34)] and st.tolist() == [18, 1, 2, 0]
    assert out[0][25] == line[25]
    # each run is interpolated between its own neighbours; sample 25 is the upper one of the first run
    # and the lower one of the second
    t = np.float32(1) / np.float32(10)
    lo, hi = np.float32(line[15].real), np.float32(line[25].real)
    assert out[0][16].real == np.float32(lo + np.float32(t * np.float32(hi - lo)))
    lo, hi = np.float32(line[25].imag), np.float32(line[35].imag)
    assert out[0][26].imag == np.float32(lo + np.float32(t * np.float32(hi - lo)))


def test_guard_zero_and_single_sample_interpolation():
    """guard 0: the run is the flagged sample alone; INTERP through a run of length 1 is the rounded
    midpoint t = 1/2 of its two neighbours."""
    ns = 64
    line = hot(quiet(ns), [7, 40])
    out, g, counts, st = R.excise(line[None], R.INTERP, 0)
    assert run_of(g[0]) == [(7, 7), (40, 40)] and st.tolist() == [2, 1, 2, 0]
    for n in (7, 40):
        lo, hi = line[n - 1], line[n + 1]
        for part in ("real", "imag"):
            a, b = np.float32(getattr(lo, part)), np.float32(getattr(hi, part))
            assert getattr(out[0][n], part) == np.float32(a + np.float32(np.float32(0.5) * np.float32(b - a)))
    assert same(out[0][~g[0]], line[~g[0]])


def test_whole_line_covered_is_zero_in_both_modes():
    """Ns 64, guard 32, flags at 16 and 48: every sample is within 32 of a flag; zeros in both modes."""
    line = hot(quiet(64), [16, 48])
    for mode in (R.ZERO, R.INTERP):
        out, g, counts, st = R.excise(line[None], mode, 32)
        assert g.all() and counts.tolist() == [64] and st.tolist() == [64, 1, 2, 1]
        assert out.tobytes() == np.zeros(64, np.complex64).tobytes()


def test_level_zero_flags_every_nonzero_sample():
    """More than half the samples zero: m = 0, T = 0, and exactly the non-zero samples are flagged."""
    line = np.zeros(64, np.complex64)
    line[[3, 4, 30, 63]] = [1e-3, 2.0 - 1.0j, 1e-20j, 5.0]
    out, g, counts, st = R.excise(line[None], R.ZERO, 0)
    assert R.level(R.power(line)) == 0.0
    assert np.flatnonzero(g[0]).tolist() == [3, 4, 30, 63] and st.tolist() == [4, 1, 4, 0]
    assert not out.any()
    sub = np.zeros(64, np.complex64)
    sub[5] = 1e-30                                 # its power underflows to +0: not flagged
    assert R.excise(sub[None], R.ZERO, 0)[3].tolist() == [0, 0, 0, 0]


def test_interpolation_through_a_long_run_int16():
    """An int16 line with a run [1, Ns - 2] (guard 0, every inner sample hot): t = j / (Ns - 1), values
    rounded half to even, inside the two neighbours' range."""
    ns = 64
    line = np.zeros((ns, 2), np.int16)
    line[1:-1] = (20000, -20000)
    line[0], line[-1] = (-7, 100), (56, 37)
    out, g, counts, st = R.excise(line[None], R.INTERP, 0, 1, 16.0)      # rank 1 %: k = 0, the smallest power
    assert run_of(g[0]) == [(1, ns - 2)] and st.tolist() == [ns - 2, 1, ns - 2, 1]
    assert same(out[0][[0, -1]], line[[0, -1]])
    for comp, (lo, hi) in enumerate(((-7, 56), (100, 37))):
        got = out[0][1:-1, comp].astype(np.int64)
        exact = lo + np.arange(1, ns - 1) * (hi - lo) / (ns - 1)
        assert np.all(np.abs(got - exact) <= 0.5 + 1e-3) and got.min() >= min(lo, hi) and got.max() <= max(lo, hi)
        assert np.all(np.diff(got) * np.sign(hi - lo) >= 0)
    want = R.brute_force(line, R.INTERP, 0, 1, 16.0)
    assert same(out[0], want[0])


def test_mask_words():
    g = np.zeros((2, 64), bool)
    g[0, [0, 31, 32]] = True
    g[1, 63] = True
    assert R.mask_words(g).tolist() == [[0x80000001, 1], [0, 0x80000000]]


# ---- synth.interference_bursts --------------------------------------------------------------------
def test_interference_bursts():
    cube = synth.frames(2, 64, 8, 2, "two_targets", seed=3)
    a, ma = synth.interference_bursts(cube, 3, 10, 5000.0, seed=9)
    b, mb = synth.interference_bursts(cube, 3, 10, 5000.0, seed=9)
    assert same(a, b) and np.array_equal(ma, mb)                         # deterministic
    c, mc = synth.interference_bursts(cube, 3, 10, 5000.0, seed=10)
    assert not np.array_equal(ma, mc)
    assert a.shape == cube.shape and a.dtype == cube.dtype and ma.shape == cube.shape and ma.dtype == bool
    assert np.array_equal(ma.sum(-1), np.broadcast_to(np.where(np.arange(8) % 3 == 0, 10, 0), (2, 2, 8)))
    for line in ma[ma.any(-1)]:
        assert R.runs_of(line)[0][1] - R.runs_of(line)[0][0] == 9 and len(R.runs_of(line)) == 1
    assert same(a[~ma], cube[~ma])                                       # nothing outside the true mask
    assert np.allclose(np.abs(a[ma] - cube[ma]), 5000.0, rtol=1e-4)
    i16 = synth.frames(1, 64, 4, 1, "two_targets", seed=3, dtype="i16")
    d, md = synth.interference_bursts(i16, 2, 64, 40000.0, seed=1)       # the whole chirp, saturating
    assert d.dtype == np.int16 and d.shape == i16.shape and md.shape == i16.shape[:-1]
    assert md[0, 0, 0].all() and not md[0, 0, 1].any() and same(d[0, 0, 1], i16[0, 0, 1])
    assert np.abs(d[0, 0, 0].astype(np.int32)).max() >= 32767
    with pytest.raises(ValueError):
        synth.interference_bursts(cube, 2, 65, 1.0, seed=1)


# ---- the CLI --------------------------------------------------------------------------------------
def test_cli_arguments(capsys):
    ap = cli.build_parser()
    a = ap.parse_args(["x.npy"])
    assert a.excise is None and a.excise_alpha == 16.0 and a.excise_guard == 4
    assert a.cfar == "os2d" and a.ca_alpha == 4.0                        # what was there is unchanged
    for mode in ("zero", "interp"):
        a = ap.parse_args(["x.npy", "--excise", mode, "--excise-alpha", "8", "--excise-guard", "2"])
        assert (a.excise, a.excise_alpha, a.excise_guard) == (mode, 8.0, 2)
    with pytest.raises(SystemExit):
        ap.parse_args(["x.npy", "--excise", "blank"])
    for flag, bad in (("--excise-alpha", "0.5"), ("--excise-alpha", "nan"), ("--excise-alpha", "inf"),
                      ("--excise-guard", "33"), ("--excise-guard", "-1")):
        with pytest.raises(SystemExit):
            cli.main(["x.npy", "--excise", "zero", flag, bad])           # rejected before the input is read
        assert flag in capsys.readouterr().err


def test_cli_without_excise_never_builds_an_exciser(monkeypatch, tmp_path, capsys):
    """Without --excise the CLI reaches RadarCore with the cube it loaded, having made no exciser; with
    it the exciser comes first."""
    made = []

    class Stop(Exception):
        pass

    class NoExciser:
        def __init__(self, *a, **k):
            made.append("exciser")
            raise Stop

    class NoCore:
        def __init__(self, *a, **k):
            made.append("core")
            raise Stop
    monkeypatch.setattr(cli, "InterferenceExciser", NoExciser)
    monkeypatch.setattr(cli, "RadarCore", NoCore)
    np.save(tmp_path / "c.npy", np.zeros((32, 64), np.complex64))
    args = [str(tmp_path / "c.npy"), "--n-range", "64", "--n-doppler", "32", "--out-dir", str(tmp_path)]
    with pytest.raises(Stop):
        cli.main(args)
    assert made == ["core"] and capsys.readouterr().out == ""
    made.clear()
    with pytest.raises(Stop):
        cli.main(args + ["--excise", "interp"])
    assert made == ["exciser"]


# ---- the end-to-end claim under the oracle ----------------------------------------------------------
def e2e_cubes():
    """64 chirps x 256 samples of unit complex Gaussian noise, one target of amplitude 0.35 at range bin
    67, Doppler bin 5, and 24-sample bursts of amplitude 100 in every second chirp."""
    nc, ns = 64, 256
    rng = np.random.default_rng(1)
    noise = (rng.standard_normal((nc, ns)) + 1j * rng.standard_normal((nc, ns))) * np.sqrt(0.5)
    n, c = np.arange(ns)[None, :], np.arange(nc)[:, None]
    clean = (noise + 0.35 * np.exp(2j * np.pi * (67 * n / ns + 5 * c / nc))).astype(np.complex64)[None, None]
    dirty, truth = synth.interference_bursts(clean, 2, 24, 100.0, seed=101)
    return clean, dirty, truth


def test_weak_target_is_found_again_after_excision():
    """Under oracle/fmcw_oracle.py (Hamming windows, |X| map, the default 2-D OS-CFAR, k = 96 of 128).
    Measured CUT / threshold at (67, 5): clean 7.22, with bursts 0.42, repaired 6.38 (zero) and 6.40
    (interp): detected iff > 1."""
    clean, dirty, truth = e2e_cubes()
    assert truth.sum() == 32 * 24

    def target(cube):
        o = O.process(cube[0], O.Cfar2D())
        cells = set(zip(o["dets"]["range"].tolist(), o["dets"]["doppler"].tolist()))
        print(f"CUT / threshold {o['mag32'][67, 5] / o['thr'][67, 5]:.2f}, {len(cells)} detections")
        return (67, 5) in cells
    assert target(clean) and not target(dirty)
    for mode in (R.ZERO, R.INTERP):
        assert R.excise(clean, mode)[3].tolist() == [0, 0, 0, 0]        # nothing flagged on the clean cube
        fixed, g, counts, st = R.excise(dirty, mode)
        assert not (truth & ~g).any() and st[2] == truth.sum() and st[1] == 32 and st[3] == 0
        assert st[0] == counts.sum() <= 32 * (24 + 8)                    # the bursts and the guard, no more
        assert same(fixed[~g], dirty[~g]) and same(dirty[~truth], clean[~truth])
        assert target(fixed), mode
