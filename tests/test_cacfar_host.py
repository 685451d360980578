"""The cell-averaging detector without a GPU: the C-ABI's layout, exports and argument checks (they come
before any device access), the specification (tests/cacfar_ref.py) against an independent brute-force
float64 mean, a hand case with exact sums, the golden 2-D CFAR map, and the CLI's arguments."""
import ctypes as C
import math
import subprocess

import numpy as np
import pytest

from fmcw import _lib as L
from fmcw import CaCfar, cli  # noqa: F401
import cacfar_ref as R

NEW_SYMBOLS = ("fmcw_cacfar_config_default", "fmcw_cacfar_create", "fmcw_cacfar_destroy", "fmcw_cacfar_enqueue",
               "fmcw_cacfar_set_grid_for_test")
WINDOWS = [((4, 4), (1, 2)), ((0, 8), (0, 2)), ((8, 0), (0, 0)), ((1, 1), (0, 0)), ((8, 8), (4, 4))]   # (ref, guard)


def default_cfg(lib):
    cfg = L.FmcwCaCfarConfig()
    lib.fmcw_cacfar_config_default(C.byref(cfg))
    return cfg


def test_layout_and_defaults(lib_built):
    assert C.sizeof(L.FmcwCaCfarConfig) == 48
    names = ["n_range", "n_doppler", "mode", "ref_range", "guard_range", "ref_doppler", "guard_doppler", "alpha",
             "max_frames", "device_id", "reserved"]
    assert [f[0] for f in L.FmcwCaCfarConfig._fields_] == names
    for i, name in enumerate(names):
        assert getattr(L.FmcwCaCfarConfig, name).offset == 4 * i
    assert L.FmcwCaCfarConfig.reserved.size == 8
    src = L.HEADER_PATH.read_text()
    body = src[src.index("typedef struct fmcw_cacfar_config {"):src.index("} fmcw_cacfar_config;")]
    decl = [n + ("[2];" if n == "reserved" else ";") for n in names]
    assert all(d in body for d in decl)                                   # every field, in this order
    assert sorted(decl, key=body.index) == decl
    assert "float alpha;" in body and "int32_t mode;" in body and "int32_t device_id;" in body
    cfg = default_cfg(lib_built)
    assert (cfg.n_range, cfg.n_doppler, cfg.mode) == (1024, 128, L.CACFAR_CA)
    assert (cfg.ref_range, cfg.guard_range, cfg.ref_doppler, cfg.guard_doppler) == (4, 1, 4, 2)
    assert (cfg.alpha, cfg.max_frames, cfg.device_id, tuple(cfg.reserved)) == (4.0, 1, 0, (0, 0))
    assert (L.CACFAR_CA, L.CACFAR_GO, L.CACFAR_SO) == (0, 1, 2)
    for name, v in (("CA", 0), ("GO", 1), ("SO", 2)):
        assert f"FMCW_CACFAR_{name} = {v}" in src
    assert lib_built.fmcw_abi_version() == 8 and "Still 8 with the cell-averaging detector" in src
    assert R.n_ref((4, 4), (1, 2)) == 128


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
    ({"n_doppler": 96}, b"n_doppler"), ({"n_doppler": 16}, b"n_doppler"), ({"n_doppler": 2048}, b"n_doppler"),
    ({"mode": 3}, b"mode"), ({"mode": -1}, b"mode"),
    ({"ref_range": 9}, b"ref_range"), ({"ref_doppler": 9}, b"ref_doppler"),
    ({"guard_range": 5}, b"guard_range"), ({"guard_doppler": 5}, b"guard_doppler"),
    ({"ref_range": 0, "ref_doppler": 0}, b"ref_"),                              # N = 0: no reference cell
    # 2 Hd + 1 > n_doppler: inside the field ranges 2 Hd + 1 <= 25 < 32, so only an extent that is
    # itself out of range gets there, and its own field is what the message names
    ({"n_doppler": 32, "ref_doppler": 14}, b"ref_doppler"), ({"n_doppler": 32, "guard_doppler": 12}, b"guard_doppler"),
    ({"n_range": 64, "ref_range": 30}, b"ref_range"),
    ({"alpha": 0.0}, b"alpha"), ({"alpha": -1.0}, b"alpha"), ({"alpha": float("nan")}, b"alpha"),
    ({"alpha": float("inf")}, b"alpha"),
    ({"max_frames": 0}, b"max_frames"), ({"max_frames": 1 << 15}, b"max_frames"),   # 2^15 x 2^17 cells = 2^32
    ({"n_range": 8192, "n_doppler": 1024, "max_frames": 512}, b"max_frames"),
    ({"reserved0": 1}, b"reserved"), ({"reserved1": 7}, b"reserved"),
    ({"device_id": -1}, b"device_id"), ({"device_id": 64}, b"device_id"),
])
def test_create_rejects_bad_fields(lib_built, fields, msg):
    cfg = default_cfg(lib_built)
    for k, v in fields.items():
        _set(cfg, k, v)
    h = C.c_void_p(1)
    rc = lib_built.fmcw_cacfar_create(C.byref(cfg), C.byref(h))
    assert rc == L.FMCW_EINVAL
    assert msg in lib_built.fmcw_last_error(), lib_built.fmcw_last_error()
    assert not h.value


def test_null_arguments(lib_built):
    assert lib_built.fmcw_cacfar_create(None, None) == L.FMCW_EINVAL
    assert lib_built.fmcw_cacfar_destroy(None) == L.FMCW_OK
    assert lib_built.fmcw_cacfar_set_grid_for_test(None, 1) == L.FMCW_EINVAL
    assert b"detector" in lib_built.fmcw_last_error()
    assert lib_built.fmcw_cacfar_enqueue(None, None, 1, None, 0, None, None) == L.FMCW_EINVAL
    lib_built.fmcw_cacfar_config_default(None)


def test_create_without_device_fails_cleanly(lib_built):
    cfg = default_cfg(lib_built)
    h = C.c_void_p(1)
    rc = lib_built.fmcw_cacfar_create(C.byref(cfg), C.byref(h))
    if L.device_count() > 0:      # a valid configuration: the GPU tests take it from here
        assert rc == L.FMCW_OK and h.value
        assert lib_built.fmcw_cacfar_destroy(h) == L.FMCW_OK
    else:
        assert rc == L.FMCW_ENODEV and not h.value


def brute_force(m, ref, guard, alpha):
    """Per tested cell, in float64 over the explicitly enumerated reference cells: (mean of all, mean
    of the upper / left half, mean of the lower / right half) x alpha.  The halves as the header
    draws them: rows above plus the left segments of the guard rows; rows below plus the right ones."""
    (rr, rd), (gr, gd) = ref, guard
    hr, hd = rr + gr, rd + gd
    nr, nd = m.shape
    m = m.astype(np.float64)
    n = R.n_ref(ref, guard)
    out = np.full((3, nr, nd), np.nan)
    for r in range(hr, nr - hr):
        for d in range(nd):
            a = b = 0.0
            na = nb = 0
            for dr in range(-hr, hr + 1):
                for dd in range(-hd, hd + 1):
                    if abs(dr) <= gr and abs(dd) <= gd:
                        continue
                    v = m[r + dr, (d + dd) % nd]
                    if dr < -gr or (abs(dr) <= gr and dd < 0):
                        a, na = a + v, na + 1
                    else:
                        b, nb = b + v, nb + 1
            assert na == nb == n // 2
            out[:, r, d] = alpha * (a + b) / n, alpha * a / na, alpha * b / nb
    return out


@pytest.mark.parametrize("ref,guard", WINDOWS)
def test_reference_against_the_definition(ref, guard):
    """cacfar_ref against the brute-force float64 means.  Every reference sum adds N non-negative
    terms in fp32, each add within half an ulp of the running sum, so the threshold is within N fp32
    ulps (N x 2^-23 relative) of the exact one; detections agree except where |m - T| / T is below
    that bound."""
    nr, nd, alpha = 32, 32, 1.0
    rng = np.random.default_rng(5)
    m = rng.rayleigh(1.0, (nr, nd)).astype(np.float32)
    n = R.n_ref(ref, guard)
    bound = n * 2.0 ** -23
    want = brute_force(m, ref, guard, alpha)
    hr = ref[0] + guard[0]
    for i, mode in enumerate(R.MODES):
        mm, t, tested = R.thresholds(m, mode, ref, guard, alpha)
        w = want[0] if mode == "ca" else np.maximum(want[1], want[2]) if mode == "go" else np.minimum(want[1], want[2])
        assert tested[hr:nr - hr].all() and not tested[:hr].any() and not tested[nr - hr:].any()
        rel = np.abs(t[tested].astype(np.float64) - w[tested]) / w[tested]
        print(f"\n{mode} {ref} {guard}: N {n}, worst threshold error {rel.max() / bound:.3f} of the bound")
        assert rel.max() <= bound
        clear = np.abs(m.astype(np.float64) - w) / w > bound
        hit = tested & (mm > t)
        assert np.array_equal(hit[tested & clear], (m > w)[tested & clear])
        dets = R.detect(m, mode, ref, guard, alpha)
        assert len(dets) == hit.sum() > 0
        key = dets["range"].astype(np.int64) * nd + dets["doppler"]
        assert np.all(np.diff(key) > 0) and not hit[:hr].any() and not hit[nr - hr:].any()


@pytest.mark.parametrize("ref,guard", WINDOWS)
def test_right_segment_is_the_left_one_shifted(ref, guard):
    """Rg[r][d] = Lg[r][d + Hd + Gd + 1] bit for bit (the same terms in the same order): what lets a
    kernel keep one of the two."""
    m = R.nonneg(np.random.default_rng(6).rayleigh(1.0, (8, 64)))
    hd, gd = ref[1] + guard[1], guard[1]
    lg, rg = R._sum(m, -1, -hd, -gd - 1), R._sum(m, -1, gd + 1, hd)
    assert np.array_equal(rg, np.roll(lg, -(hd + gd + 1), axis=-1))


def test_hand_case():
    """An 8 x 8 integer map, window 1/0/1/0 (N = 8), alpha 2: every sum is exact, so the thresholds
    are the integers' own: T = 2 x (sum of the 8 neighbours) / 8 for CA, 2 x (half sum) / 4 for GO / SO."""
    m = np.array([[1, 2, 3, 4, 5, 6, 7, 8],
                  [8, 7, 6, 5, 4, 3, 2, 1],
                  [1, 1, 40, 1, 1, 1, 1, 9],
                  [2, 2, 2, 2, 2, 2, 2, 2],
                  [3, 0, 3, 0, 3, 0, 3, 0],
                  [9, 1, 1, 1, 1, 30, 1, 1],
                  [4, 4, 4, 4, 4, 4, 4, 4],
                  [5, 6, 7, 8, 1, 2, 3, 4]], np.float32)
    want = {}
    for mode in R.MODES:
        t = np.zeros((8, 8))
        for r in range(1, 7):
            for d in range(8):
                a = m[r - 1, (d - 1) % 8] + m[r - 1, d] + m[r - 1, (d + 1) % 8] + m[r, (d - 1) % 8]
                b = m[r + 1, (d - 1) % 8] + m[r + 1, d] + m[r + 1, (d + 1) % 8] + m[r, (d + 1) % 8]
                t[r, d] = 2 * (a + b) / 8 if mode == "ca" else 2 * max(a, b) / 4 if mode == "go" else 2 * min(a, b) / 4
        want[mode] = t
        _, got, tested = R.thresholds(m, mode, (1, 1), (0, 0), 2.0)
        assert np.array_equal(got[tested].astype(np.float64), t[1:7].ravel())
        dets = R.detect(m, mode, (1, 1), (0, 0), 2.0)
        cells = [(r, d) for r in range(1, 7) for d in range(8) if m[r, d] > t[r, d]]
        assert list(zip(dets["range"].tolist(), dets["doppler"].tolist())) == cells
        assert (2, 2) in cells and (5, 5) in cells
        assert np.array_equal(dets["mag"], [m[c] for c in cells])
        assert np.array_equal(dets["threshold"].astype(np.float64), [t[c] for c in cells])
    assert (2, 7) in [(r, d) for r in range(1, 7) for d in range(8) if m[r, d] > want["so"][r, d]]   # the wrap: d = 7 sees d = 0


def test_negative_cells_enter_as_zero():
    m = np.array([[-1.0, -0.0, 0.0, 2.0]], np.float32)
    got = R.nonneg(m)
    assert np.array_equal(got.view(np.uint32), np.array([[0, 0, 0, 0x40000000]], np.uint32))
    assert R.nonneg(np.array([np.inf], np.float32))[0] == np.inf


def test_golden_cfar2d_map(golden):
    """tests/golden/tb_cfar2d.npz (64 x 32), window 3/1/2/1, alpha 4: all three modes detect exactly
    the 18 cells of the two 3 x 3 targets."""
    m = np.load(golden / "tb_cfar2d.npz")["map"].astype(np.float32)
    cells = [(r, d) for r0, d0 in ((30, 16), (50, 8)) for r in (r0 - 1, r0, r0 + 1) for d in (d0 - 1, d0, d0 + 1)]
    for mode in R.MODES:
        dets = R.detect(m, mode, (3, 2), (1, 1), 4.0)
        assert list(zip(dets["range"].tolist(), dets["doppler"].tolist())) == sorted(cells), mode
        assert np.all(dets["frame"] == 0) and np.all(dets["mag"] > dets["threshold"])


def test_python_class_and_constants(lib_built):
    assert CaCfar.__init__.__defaults__ == (1024, 128, "ca", (4, 4), (1, 2), 4.0, 1, 0)
    for name in ("enqueue", "detect", "set_grid_for_test", "close", "__enter__", "__exit__"):
        assert callable(getattr(CaCfar, name))
    with pytest.raises(KeyError):
        CaCfar(64, 32, mode="os")
    with pytest.raises(L.FmcwError, match="ref_range"):
        CaCfar(64, 32, ref=(9, 4))
    assert math.isclose(np.float32(np.float64(np.float32(4.0)) / 128), 0.03125)


def test_cli_arguments(capsys):
    ap = cli.build_parser()
    a = ap.parse_args(["x.npy"])
    assert a.cfar == "os2d" and a.ca_alpha == 4.0
    for kind in ("ca", "go", "so"):
        assert ap.parse_args(["x.npy", "--cfar", kind, "--ca-alpha", "2.5"]).ca_alpha == 2.5
        assert ap.parse_args(["x.npy", "--cfar", kind]).cfar == kind
    with pytest.raises(SystemExit):
        ap.parse_args(["x.npy", "--cfar", "cago"])
    for bad in ("-1", "0", "nan", "inf"):
        with pytest.raises(SystemExit):
            cli.main(["x.npy", "--cfar", "ca", "--ca-alpha", bad])           # rejected before the input is read
        assert "--ca-alpha" in capsys.readouterr().err
