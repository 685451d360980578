"""Beam merge, host side (no GPU): the C-ABI's layouts and argument checks (validated before any
device access), the specification itself -- tests/merge_ref.py pinned against plots_ref.py, on
hand-made lists, and on a small multi-channel scene through the references alone.
"""
import ctypes as C
import functools
import subprocess

import numpy as np
import pytest

import fmcw_oracle as O
from fmcw import DET_DTYPE, MPLOT_DTYPE, PLOT_DTYPE, BeamMerger, steering_weights
from fmcw import _lib as L
from fmcw import merge as M
from beams_ref import beams_ref
from merge_ref import HAND, hand_records, merge_ref, random_list, tile_edge_list
from plots_ref import plots_ref
from tile_edge import TILE_EDGE_SIZES

NEW_SYMBOLS = ("fmcw_merge_config_default", "fmcw_merge_create", "fmcw_merge_destroy", "fmcw_merge_enqueue",
               "fmcw_merge_set_grid_for_test")
FIELDS = ["n_range", "n_doppler", "n_beams", "win_beam", "win_range", "win_doppler", "beam_wrap", "max_recs",
          "max_maps", "device_id"]
ONE = C.c_void_p(0x1000)   # a non-null, aligned stand-in: the checks below never dereference it


def default_cfg(lib):
    cfg = L.FmcwMergeConfig()
    lib.fmcw_merge_config_default(C.byref(cfg))
    return cfg


def test_layouts_defaults_and_abi(lib_built):
    assert C.sizeof(L.FmcwMplot) == 32 and C.sizeof(L.FmcwMergeConfig) == 40
    offs = {n: getattr(L.FmcwMplot, n).offset for n, _ in L.FmcwMplot._fields_}
    assert offs == {"frame": 0, "range": 4, "doppler": 6, "mag": 8, "beam": 12, "n_merged": 14, "sum_mag": 16,
                    "d_beam": 20, "d_range": 24, "d_doppler": 28}
    assert MPLOT_DTYPE.itemsize == 32 and {n: MPLOT_DTYPE.fields[n][1] for n in MPLOT_DTYPE.names} == offs
    # the tracker and the bearing estimator read frame / range / doppler / mag where fmcw_plot has them
    for n in ("frame", "range", "doppler", "mag"):
        assert MPLOT_DTYPE.fields[n] == PLOT_DTYPE.fields[n]
    assert [f[0] for f in L.FmcwMergeConfig._fields_] == FIELDS
    assert [getattr(L.FmcwMergeConfig, n).offset for n in FIELDS] == list(range(0, 40, 4))
    src = L.HEADER_PATH.read_text()
    body = src[src.index("typedef struct fmcw_merge_config {"):src.index("} fmcw_merge_config;")]
    assert sorted(FIELDS, key=lambda n: body.index(f" {n};")) == FIELDS
    assert "#define FMCW_MERGE_STATUS_WORDS 3" in src and L.MERGE_STATUS_WORDS == 3
    cfg = default_cfg(lib_built)
    assert [getattr(cfg, n) for n in FIELDS] == [1024, 128, 1, 1, 1, 1, 0, 1 << 20, 1024, 0]
    assert lib_built.fmcw_abi_version() == 8 and "Still 8 with the beam merge" in src


def test_new_symbols_exported(lib_built):
    out = subprocess.run(["nm", "-D", "--defined-only", str(L.LIB_PATH)], capture_output=True, text=True,
                         check=True).stdout
    src = L.HEADER_PATH.read_text()
    for name in NEW_SYMBOLS:
        assert f" T {name}\n" in out, name
        assert name in L.SIGNATURES and f"{name}(" in src


@pytest.mark.parametrize("fields,msg", [
    (dict(n_range=0), b"n_range"), (dict(n_range=65537), b"n_range"),
    (dict(n_doppler=2), b"n_doppler"), (dict(n_doppler=8, win_doppler=4), b"n_doppler"), (dict(n_doppler=65537), b"n_doppler"),
    (dict(n_beams=0), b"n_beams"), (dict(n_beams=65, max_maps=65), b"n_beams"),
    (dict(win_beam=5), b"win_beam"), (dict(win_range=5), b"win_range"), (dict(win_doppler=5), b"win_doppler"),
    (dict(beam_wrap=2), b"beam_wrap"), (dict(beam_wrap=1, n_beams=2, max_maps=2), b"beam_wrap"),
    (dict(beam_wrap=1, n_beams=8, win_beam=4, max_maps=8), b"beam_wrap"),
    (dict(max_recs=0), b"max_recs"), (dict(max_recs=1 << 31), b"max_recs"),
    (dict(max_maps=0), b"max_maps"), (dict(n_beams=3, max_maps=1024), b"max_maps"), (dict(n_beams=8, max_maps=4), b"max_maps"),
    (dict(max_maps=1 << 31), b"max_maps"),
    (dict(device_id=64), b"device_id"), (dict(device_id=-1), b"device_id"),
])
def test_create_rejects_bad_config(lib_built, fields, msg):
    cfg = default_cfg(lib_built)
    for k, v in fields.items():
        setattr(cfg, k, v)
    h = C.c_void_p(1)
    assert lib_built.fmcw_merge_create(C.byref(cfg), C.byref(h)) == L.FMCW_EINVAL
    assert msg in lib_built.fmcw_last_error(), lib_built.fmcw_last_error()
    assert not h.value


def test_null_arguments(lib_built):
    lib = lib_built
    lib.fmcw_merge_config_default(None)            # ignored
    cfg = default_cfg(lib)
    h = C.c_void_p()
    assert lib.fmcw_merge_create(None, C.byref(h)) == L.FMCW_EINVAL
    assert lib.fmcw_merge_create(C.byref(cfg), None) == L.FMCW_EINVAL
    assert lib.fmcw_merge_destroy(None) == L.FMCW_OK
    assert lib.fmcw_merge_set_grid_for_test(None, 1) == L.FMCW_EINVAL and lib.fmcw_last_error() == b"null merger"


@pytest.mark.parametrize("kw,msg", [
    (dict(rec_stride=8), b"rec_stride"), (dict(rec_stride=24), b"rec_stride"), (dict(rec_stride=0), b"rec_stride"),
    (dict(rec_stride=64), b"rec_stride"),
    (dict(recs=None), b"recs_dev"), (dict(n_recs=None), b"n_recs_dev"), (dict(out=None), b"out_dev"),
    (dict(status=None), b"status_dev"),
    (dict(out=C.c_void_p(0x1008)), b"out_dev must be 16-byte aligned"),
    (dict(recs=C.c_void_p(0x1004)), b"recs_dev must be 16-byte aligned"),
    (dict(), b"null merger"),
])
def test_enqueue_checks_arguments_before_the_merger(lib_built, kw, msg):
    """Everything that does not depend on the merger is checked first, so these hold with a null
    merger on a machine without a device."""
    a = dict(recs=ONE, rec_stride=16, rec_cap=4, n_recs=ONE, n_maps=1, out=ONE, out_cap=4, status=ONE)
    a.update(kw)
    rc = lib_built.fmcw_merge_enqueue(None, a["recs"], a["rec_stride"], a["rec_cap"], a["n_recs"], a["n_maps"],
                                      a["out"], a["out_cap"], a["status"], None)
    assert rc == L.FMCW_EINVAL
    assert msg in lib_built.fmcw_last_error(), lib_built.fmcw_last_error()


def test_create_without_device_and_n_maps_limits(lib_built):
    """Without a device a valid configuration is FMCW_ENODEV; with one, n_maps above max_maps or no
    multiple of n_beams is FMCW_EINVAL naming n_maps before anything is launched (the pointers are
    never dereferenced)."""
    cfg = default_cfg(lib_built)
    cfg.n_beams, cfg.max_maps = 3, 6
    h = C.c_void_p(1)
    rc = lib_built.fmcw_merge_create(C.byref(cfg), C.byref(h))
    if L.device_count() < 1:
        assert rc == L.FMCW_ENODEV and not h.value
        return
    assert rc == L.FMCW_OK and h.value
    try:
        for n_maps, text in ((9, b"max_maps"), (4, b"n_beams")):
            assert lib_built.fmcw_merge_enqueue(h, ONE, 16, 4, ONE, n_maps, ONE, 4, ONE, None) == L.FMCW_EINVAL
            assert b"n_maps" in lib_built.fmcw_last_error() and text in lib_built.fmcw_last_error()
    finally:
        assert lib_built.fmcw_merge_destroy(h) == L.FMCW_OK


def test_python_class(lib_built):
    assert BeamMerger.__init__.__defaults__ == (1024, 128, 1, (1, 1, 1), False, 1 << 20, None, 0)
    for name in ("enqueue", "merge", "beam_position", "interp", "set_grid_for_test", "close"):
        assert callable(getattr(BeamMerger, name))
    with pytest.raises(L.FmcwError, match="win_beam"):
        BeamMerger(64, 32, 4, win=(5, 1, 1))
    p = np.zeros(3, MPLOT_DTYPE)
    p["beam"], p["d_beam"] = [0, 3, 7], [-0.25, 0.5, 0.75]
    np.testing.assert_allclose(M.beam_position(p, 8), [-0.25, 3.5, 7.75])
    np.testing.assert_allclose(M.beam_position(p, 8, True), [7.75, 3.5, 7.75])
    u = (np.arange(8) - 4) / 8.0
    np.testing.assert_allclose(M.interp(p, u), [-0.5, -0.0625, 0.375])           # held at the ends
    np.testing.assert_allclose(M.interp(p, u, True, period=1.0), [0.46875, -0.0625, 0.46875])


@pytest.mark.parametrize("n", TILE_EDGE_SIZES)
def test_tile_edge_lists_have_merged_plots(n):
    want, beyond = merge_ref(tile_edge_list(n), 32, 32, 3, (1, 1, 1), False, 6)
    assert beyond == 0 and len(want) > 0


@pytest.mark.parametrize("win", [(1, 1), (0, 3), (4, 4), (2, 1)])
def test_reference_equals_plots_ref_on_one_beam(win):
    """n_beams = 1, win_beam = 0: the merger's specification is the plot extractor's."""
    dets = random_list(21, 3, 32, 16, 0.4)
    p = plots_ref(dets, 32, 16, *win)
    m, beyond = merge_ref(dets, 32, 16, 1, (0, *win))
    assert beyond == 0 and len(m) == len(p) > 0
    for a, b in (("frame", "frame"), ("range", "range"), ("doppler", "doppler"), ("mag", "mag"),
                 ("n_merged", "n_cells"), ("sum_mag", "sum_mag"), ("d_range", "d_range"), ("d_doppler", "d_doppler")):
        np.testing.assert_array_equal(m[a], p[b], err_msg=a)
    assert not m["beam"].any() and not m["d_beam"].any()


@pytest.mark.parametrize("name", sorted(HAND))
def test_reference_hand_cases(name):
    rows, win, wrap, want = HAND[name]
    m, _ = merge_ref(hand_records(rows, DET_DTYPE), 8, 8, 3, win, bool(wrap))
    got = [tuple(int(p[k]) for k in ("frame", "beam", "range", "doppler", "n_merged")) for p in m]
    assert got == want
    if name == "same_cell_three_beams":
        assert m["d_beam"][0] == (-2.0 + 1.0) / 8.0 and m["sum_mag"][0] == 8.0
    if name == "doppler_wrap":
        assert m["d_doppler"][0] == pytest.approx(2.0 / 7.0) and m["d_beam"][0] == pytest.approx(-2.0 / 7.0)
    if name == "share_cell_wrap_w1":
        assert m["d_beam"][0] == pytest.approx(-4.0 / 9.0)    # beam 2 is one beam below beam 0 on the circle


# ---- the references alone on a small multi-channel scene ----
NRX, NB, NR, NC = 8, 8, 128, 32
NUS = (np.arange(NB) - NB // 2) / NB           # DFT beams: nu = (b - 4) / 8 cycles per element
# (range, doppler, nu, amplitude): one target between beams 4 and 5, two in one cell three beams apart
TARGETS = [(40, 9, 0.05, 6.0), (90, 20, -0.375, 5.0), (90, 20, 0.0, 7.0)]


def true_beam(nu):
    return (nu * NB + NB // 2) % NB


@functools.lru_cache(maxsize=None)
def physical_scene():
    """(range spectrum [1][rx][range][chirp], the per-beam plots as one PLOT list)."""
    rng = np.random.default_rng(5)
    spec = 0.05 * (rng.standard_normal((1, NRX, NR, NC)) + 1j * rng.standard_normal((1, NRX, NR, NC)))
    c, k = np.arange(NC), np.arange(NRX)
    for r, d, nu, amp in TARGETS:
        spec[0, :, r, :] += amp * np.exp(2j * np.pi * (d * c[None, :] / NC + nu * k[:, None]))
    spec = spec.astype(np.complex64)
    maps, _ = beams_ref(spec, steering_weights(NRX, NUS))
    maps = maps.astype(np.float32).reshape(NB, NR, NC)
    plots = []
    for m in range(NB):
        det, thr = O.cfar_os1d(maps[m], O.Cfar1D())
        plots.append(plots_ref(O.detections(det, maps[m], thr, frame=m), NR, NC, 1, 1))
    return spec, np.concatenate(plots)


def test_physical_scene_through_the_references():
    """beams_ref -> the oracle's 1-D OS-CFAR -> plots_ref per map -> merge_ref on 8 channels, 8 DFT
    beams, 128 x 32: per-beam plot extraction leaves more than one plot per target; the merge
    leaves exactly one, and its beam position is within 0.5 beam of the target's own."""
    _, plots = physical_scene()
    merged, beyond = merge_ref(plots, NR, NC, NB, (1, 1, 1), True)
    assert beyond == 0
    assert len(plots) > len(TARGETS) and len(merged) == len(TARGETS)
    pos = M.beam_position(merged, NB, True)
    for r, d, nu, _ in TARGETS:
        hit = [i for i in range(len(merged)) if merged["range"][i] == r and merged["doppler"][i] == d
               and abs((pos[i] - true_beam(nu) + NB / 2) % NB - NB / 2) <= 0.5]
        assert len(hit) == 1, (r, d, nu, merged, pos)
        err = (pos[hit[0]] - true_beam(nu) + NB / 2) % NB - NB / 2
        print(f"target nu {nu:+.3f}: beam position {pos[hit[0]]:.3f}, true {true_beam(nu):.3f}, error {err:+.3f}")
    between = merged[(merged["range"] == 40)][0]
    assert between["n_merged"] >= 2          # seen in more than one beam
