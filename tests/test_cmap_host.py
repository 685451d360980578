"""The clutter map without a GPU: the C-ABI's layout, exports and argument checks (they come before any
device access), the properties of the specification (tests/cmap_ref.py), and the clutter-edge case on
which a scan-to-scan threshold finds a target that the cell-averaging detector's spatial window misses."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from fmcw import _lib as L
from fmcw import ClutterMap
import cacfar_ref as CA
import cmap_ref as R

NEW_SYMBOLS = ("fmcw_cmap_config_default", "fmcw_cmap_create", "fmcw_cmap_destroy", "fmcw_cmap_enqueue",
               "fmcw_cmap_reset", "fmcw_cmap_get_state", "fmcw_cmap_set_state", "fmcw_cmap_set_grid_for_test")
FIELDS = ["n_range", "n_doppler", "n_streams", "gain", "alpha", "floor", "clip", "spread_range", "spread_doppler",
          "warmup", "max_frames", "device_id", "reserved"]


def default_cfg(lib):
    cfg = L.FmcwCmapConfig()
    lib.fmcw_cmap_config_default(C.byref(cfg))
    return cfg


def test_layout_and_defaults(lib_built):
    assert C.sizeof(L.FmcwCmapConfig) == 64
    assert [f[0] for f in L.FmcwCmapConfig._fields_] == FIELDS
    for i, name in enumerate(FIELDS):
        assert getattr(L.FmcwCmapConfig, name).offset == 4 * i
    assert L.FmcwCmapConfig.reserved.size == 16
    src = L.HEADER_PATH.read_text()
    body = src[src.index("typedef struct fmcw_cmap_config {"):src.index("} fmcw_cmap_config;")]
    decl = [n + ("[4];" if n == "reserved" else ";") for n in FIELDS]
    assert all(d in body for d in decl)
    assert sorted(decl, key=body.index) == decl                           # every field, in this order
    for f in ("gain", "alpha", "floor", "clip"):
        assert f"float {f};" in body
    assert "int32_t device_id;" in body and "uint32_t warmup;" in body
    cfg = default_cfg(lib_built)
    assert (cfg.n_range, cfg.n_doppler, cfg.n_streams) == (1024, 128, 1)
    assert (cfg.gain, cfg.alpha, cfg.floor, cfg.clip) == (0.125, 4.0, 0.0, 0.0)
    assert (cfg.spread_range, cfg.spread_doppler, cfg.warmup, cfg.max_frames, cfg.device_id) == (1, 1, 8, 1, 0)
    assert tuple(cfg.reserved) == (0, 0, 0, 0)
    assert lib_built.fmcw_abi_version() == 8 and "Still 8 with the clutter map" in src
    assert R.DEFAULTS == dict(n_streams=1, gain=0.125, alpha=4.0, floor=0.0, clip=0.0, spread=(1, 1), warmup=8)


def test_new_symbols_exported(lib_built):
    out = subprocess.run(["nm", "-D", "--defined-only", str(L.LIB_PATH)], capture_output=True, text=True,
                         check=True).stdout
    src = L.HEADER_PATH.read_text()
    for name in NEW_SYMBOLS:
        assert f" T {name}\n" in out, name
        assert name in L.SIGNATURES and f"{name}(" in src


def _set(cfg, field, value):
    if field.startswith("reserved"):
        cfg.reserved[int(field[-1])] = value
    else:
        setattr(cfg, field, value)


@pytest.mark.parametrize("fields,msg", [
    ({"n_range": 1000}, b"n_range"), ({"n_range": 32}, b"n_range"), ({"n_range": 16384}, b"n_range"),
    ({"n_doppler": 96}, b"n_doppler"), ({"n_doppler": 16}, b"n_doppler"), ({"n_doppler": 2048}, b"n_doppler"),
    ({"n_streams": 0}, b"n_streams"), ({"n_streams": 65, "max_frames": 65}, b"n_streams"),
    ({"gain": 0.0}, b"gain"), ({"gain": -0.5}, b"gain"), ({"gain": 1.5}, b"gain"), ({"gain": float("nan")}, b"gain"),
    ({"gain": float("inf")}, b"gain"),
    ({"alpha": 0.0}, b"alpha"), ({"alpha": -1.0}, b"alpha"), ({"alpha": float("nan")}, b"alpha"),
    ({"alpha": float("inf")}, b"alpha"),
    ({"floor": -1.0}, b"floor"), ({"floor": float("nan")}, b"floor"), ({"floor": float("inf")}, b"floor"),
    ({"clip": 0.5}, b"clip"), ({"clip": -2.0}, b"clip"), ({"clip": float("nan")}, b"clip"),
    ({"clip": float("inf")}, b"clip"),
    ({"spread_range": 5}, b"spread_range"), ({"spread_doppler": 5}, b"spread_doppler"),
    ({"spread_doppler": 1 << 31}, b"spread_doppler"),
    ({"warmup": 0}, b"warmup"),
    ({"max_frames": 0}, b"max_frames"), ({"n_streams": 3, "max_frames": 4}, b"max_frames"),
    ({"n_streams": 4, "max_frames": 2}, b"max_frames"),
    ({"max_frames": 1 << 15}, b"max_frames"),                                       # 2^15 x 2^17 cells = 2^32
    ({"n_range": 8192, "n_doppler": 1024, "max_frames": 512}, b"max_frames"),
    ({"reserved0": 1}, b"reserved"), ({"reserved3": 7}, b"reserved"),
    ({"device_id": -1}, b"device_id"), ({"device_id": 64}, b"device_id"),
])
def test_create_rejects_bad_fields(lib_built, fields, msg):
    cfg = default_cfg(lib_built)
    for k, v in fields.items():
        _set(cfg, k, v)
    h = C.c_void_p(1)
    rc = lib_built.fmcw_cmap_create(C.byref(cfg), C.byref(h))
    assert rc == L.FMCW_EINVAL
    assert msg in lib_built.fmcw_last_error(), lib_built.fmcw_last_error()
    assert not h.value


def test_null_arguments(lib_built):
    assert lib_built.fmcw_cmap_create(None, None) == L.FMCW_EINVAL
    assert lib_built.fmcw_cmap_destroy(None) == L.FMCW_OK
    for rc in (lib_built.fmcw_cmap_set_grid_for_test(None, 1), lib_built.fmcw_cmap_reset(None, None),
               lib_built.fmcw_cmap_get_state(None, None, None, None), lib_built.fmcw_cmap_set_state(None, None, None, None),
               lib_built.fmcw_cmap_enqueue(None, None, 1, None, 0, None, None)):
        assert rc == L.FMCW_EINVAL
        assert b"clutter map" in lib_built.fmcw_last_error()
    lib_built.fmcw_cmap_config_default(None)


def test_create_without_device_fails_cleanly(lib_built):
    cfg = default_cfg(lib_built)
    h = C.c_void_p(1)
    rc = lib_built.fmcw_cmap_create(C.byref(cfg), C.byref(h))
    if L.device_count() > 0:      # a valid configuration: the GPU tests take it from here
        assert rc == L.FMCW_OK and h.value
        assert lib_built.fmcw_cmap_destroy(h) == L.FMCW_OK
    else:
        assert rc == L.FMCW_ENODEV and not h.value


def test_python_class(lib_built):
    assert ClutterMap.__init__.__defaults__ == (1024, 128, 1, 0.125, 4.0, 0.0, 0.0, (1, 1), 8, 1, 0)
    for name in ("enqueue", "detect", "reset", "get_state", "set_state", "set_grid_for_test", "close", "__enter__",
                 "__exit__"):
        assert callable(getattr(ClutterMap, name))
    with pytest.raises(L.FmcwError, match="spread_range"):
        ClutterMap(64, 32, spread=(5, 1))


# ---- the specification's properties ----

def noise(shape, seed):
    """Writable Rayleigh(1) noise of any shape (gpu_support.rayleigh is the cached, read-only 3-D one)."""
    return np.random.default_rng(seed).rayleigh(1.0, shape).astype(np.float32)


def test_first_scan_initialises_and_warmup_holds_detections_back():
    maps = noise((6, 16, 32), 1)
    maps[:, 5, 7] = [1, 1, 1, 50, 60, 70]
    dets, planes, ages = R.detect(maps[:1], warmup=1)
    assert len(dets) == 0 and ages.tolist() == [1]
    assert planes[0].tobytes() == R.nonneg(maps[0]).tobytes()          # c' = x
    for warmup in (1, 3, 5):
        dets, _, ages = R.detect(maps, alpha=1.0, warmup=warmup)
        assert ages.tolist() == [6]
        assert len(dets) > 0 and dets["frame"].min() == warmup        # alpha 1: about half the cells of every tested scan
        assert set(dets["frame"].tolist()) == set(range(warmup, 6))
        key = (dets["frame"].astype(np.int64) * 16 + dets["range"]) * 32 + dets["doppler"]
        assert np.all(np.diff(key) > 0)
    strong = R.detect(maps, alpha=4.0, warmup=3)[0]
    assert {(3, 5, 7), (4, 5, 7), (5, 5, 7)} <= set(zip(strong["frame"].tolist(), strong["range"].tolist(),
                                                        strong["doppler"].tolist()))


def test_constant_map_converges_to_itself_and_never_detects():
    m = noise((16, 32), 2)
    maps = np.broadcast_to(m, (20, 16, 32))
    for alpha in (1.0, 2.5):
        dets, planes, ages = R.detect(maps, alpha=alpha, warmup=1)
        assert len(dets) == 0                                  # x = c <= M <= alpha M: never x > T
        assert planes[0].tobytes() == m.tobytes() and ages.tolist() == [20]
    # from another start the recurrence contracts towards the map: |c' - x| <= (1 - g) |c - x| up to rounding
    start = (noise((1, 16, 32), 3), np.array([5], np.uint32))
    _, planes, _ = R.detect(maps, gain=0.5, warmup=100, state=start)
    assert np.abs(planes[0] - m).max() <= np.abs(start[0][0] - m).max() * 0.5 ** 20 + 4 * np.finfo(np.float32).eps * m.max()


def test_clip_bounds_the_growth_per_scan():
    base = np.full((16, 32), 2.0, np.float32)
    maps = np.stack([base] + [base.copy() for _ in range(4)])
    maps[1:, 3, 3] = 1000.0
    _, free, _ = R.detect(maps, gain=0.5, warmup=100)
    assert free[0][3, 3] > 900.0                                            # unclipped: burnt in after 4 scans
    c = np.float32(2.0)
    for k in range(1, 5):
        _, planes, _ = R.detect(maps[:k + 1], gain=0.5, clip=2.0, warmup=100)
        c = c + np.float32(0.5) * (np.minimum(np.float32(1000.0), np.float32(2.0) * c) - c)   # u = clip c
        assert planes[0][3, 3] == c == np.float32(2.0 * 1.5 ** k)          # grows by (1 + g (clip - 1)) per scan
    # the floor is the least clip level: a cell at 0 can still rise
    z = np.zeros((3, 16, 32), np.float32)
    z[1:, 2, 2] = 9.0
    assert R.detect(z, gain=1.0, clip=2.0, floor=0.0, warmup=100)[1][0][2, 2] == 0.0
    assert R.detect(z, gain=1.0, clip=2.0, floor=3.0, warmup=100)[1][0][2, 2] == 6.0        # 0 -> 3 -> min(9, 6)


def test_splitting_the_calls_changes_nothing():
    maps = noise((12, 16, 32), 4)
    kw = dict(n_streams=2, alpha=1.5, clip=3.0, floor=0.25, spread=(2, 3), warmup=2)
    whole, planes, ages = R.detect(maps, **kw)
    assert len(whole) > 0 and ages.tolist() == [6, 6]
    state, parts, off = None, [], 0
    for n in (2, 4, 6):
        d, p, a = R.detect(maps[off:off + n], state=state, **kw)
        d["frame"] += off
        parts.append(d)
        state, off = (p, a), off + n
    assert np.concatenate(parts).tobytes() == whole.tobytes()
    assert state[0].tobytes() == planes.tobytes() and state[1].tolist() == ages.tolist()
    # streams are independent: each equals a single-stream run on its own frames
    for b in range(2):
        one, p1, a1 = R.detect(maps[b::2], **dict(kw, n_streams=1))
        sel = whole[whole["frame"] % 2 == b]
        assert np.array_equal(sel["frame"] // 2, one["frame"])
        assert all(sel[k].tobytes() == one[k].tobytes() for k in ("range", "doppler", "mag", "threshold"))
        assert p1[0].tobytes() == planes[b].tobytes()


def test_neighbourhood_clips_in_range_and_wraps_in_doppler():
    c = np.zeros((8, 32), np.float32)
    c[0, 0], c[7, 31] = 5.0, 7.0
    m = R.neighbourhood_max(c, (1, 1))
    assert {tuple(x) for x in np.argwhere(m == 5.0)} == {(r, d) for r in (0, 1) for d in (31, 0, 1)}   # no row -1 -> 7
    assert {tuple(x) for x in np.argwhere(m == 7.0)} == {(r, d) for r in (6, 7) for d in (30, 31, 0)}
    brute = np.zeros_like(c)
    c2 = noise((8, 32), 5)
    for r in range(8):
        for d in range(32):
            brute[r, d] = max(c2[rr, (d + dd) % 32] for rr in range(max(r - 2, 0), min(r + 2, 7) + 1) for dd in range(-3, 4))
    assert np.array_equal(R.neighbourhood_max(c2, (2, 3)), brute)
    assert R.detect(np.zeros((2, 8, 32), np.float32), warmup=1, state=(np.zeros((1, 8, 32), np.float32), [AGE]))[2][0] == AGE


AGE = R.AGE_MAX


# ---- the clutter edge ----

def test_clutter_edge_target():
    """Rayleigh clutter whose scale steps from 4 to 1 at range row 133 of 1024 (the sea clutter of the
    reference's tb_tactical stops dead there), 32 Doppler bins, 8 warm-up scans, then a target of amplitude
    14 two rows beyond the edge, at (135, 9).

    Cell-averaging, default window 4/1/4/2, CUT row 135: 3 of its 10 full reference rows (130..132) lie in
    the strong clutter, so its mean is about 1.25 (0.3 x 4 + 0.7) = 2.4 instead of 1.25.  It needs alpha 8
    to stay free of false alarms on the strong side of the edge (row 132: T = 8 x 1.25 x 2.35 = 5.9 sigma,
    at alpha 4 that is 2.9 sigma, about 1 % per cell), and alpha 8 puts T near 19 at the target: missed.
    Clutter map, alpha 5, spread 1/1: rows 134..136 have only ever seen the weak clutter, M is about 1.8, T
    about 9: found.  Its false-alarm threshold is >= 5 x 1.25 sigma = 6.2 sigma everywhere (2e-9 per cell)."""
    nr, nd, edge, warm, amp = 1024, 32, 133, 8, 14.0
    tr, td = edge + 2, 9
    scale = np.where(np.arange(nr) < edge, 4.0, 1.0).astype(np.float32)[None, :, None]
    maps = noise((warm + 1, nr, nd), 20) * scale
    maps[warm, tr, td] = amp
    cm, _, ages = R.detect(maps, alpha=5.0, warmup=warm)
    ca = CA.detect(maps[warm], "ca", alpha=8.0)
    cells = lambda d: list(zip(d["range"].tolist(), d["doppler"].tolist()))   # noqa: E731
    t_ca = CA.thresholds(maps[warm], "ca", alpha=8.0)[1][tr, td]
    print(f"\nclutter map: {cells(cm)}, T {cm['threshold'].tolist()}; CA alpha 8: {cells(ca)}, T at the target {t_ca:.2f}")
    assert ages.tolist() == [warm + 1]
    assert cells(cm) == [(tr, td)] and cm["frame"].tolist() == [warm]         # found, and no false alarm
    assert cells(ca) == []                                                    # missed, and no false alarm
    assert cm["threshold"][0] * 1.25 < amp < t_ca / 1.25                      # both with margin
    # the same detector finds the same target away from the edge: the miss is the edge's doing
    far = maps[warm].copy()
    far[tr, td], far[600, td] = maps[warm - 1, tr, td], amp
    assert cells(CA.detect(far, "ca", alpha=8.0)) == [(600, td)]
