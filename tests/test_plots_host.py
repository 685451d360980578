"""Plot extraction, host side (no GPU): the C-ABI's layouts and argument checks
(fmcw_plots_create validates before any device access), and the specification itself -- the NumPy
restatement tests/plots_ref.py on the fp64 oracle's detections of the two_targets stimulus.
"""
import ctypes as C

import numpy as np
import pytest

import fmcw_oracle as O
from fmcw import _lib as L
from fmcw import synth
from plots_ref import plots_ref


def test_plot_struct_layouts():
    assert C.sizeof(L.FmcwPlot) == 32 and C.sizeof(L.FmcwPlotsConfig) == 24
    offs = {n: getattr(L.FmcwPlot, n).offset for n, _ in L.FmcwPlot._fields_}
    assert offs == {"frame": 0, "range": 4, "doppler": 6, "mag": 8, "threshold": 12, "n_cells": 16,
                    "sum_mag": 20, "d_range": 24, "d_doppler": 28}
    coffs = [getattr(L.FmcwPlotsConfig, n).offset for n, _ in L.FmcwPlotsConfig._fields_]
    assert coffs == [0, 4, 8, 12, 16, 20]
    from fmcw import PLOT_DTYPE
    assert PLOT_DTYPE.itemsize == 32
    assert {n: PLOT_DTYPE.fields[n][1] for n in PLOT_DTYPE.names} == offs
    src = L.HEADER_PATH.read_text()
    assert "#define FMCW_PLOT_STATUS_WORDS 2" in src and L.PLOT_STATUS_WORDS == 2


def test_plots_config_default(lib_built):
    cfg = L.FmcwPlotsConfig()
    lib_built.fmcw_plots_config_default(C.byref(cfg))
    assert (cfg.n_range, cfg.n_doppler, cfg.win_range, cfg.win_doppler, cfg.max_dets, cfg.device_id) == \
        (1024, 128, 1, 1, 1 << 20, 0)


@pytest.mark.parametrize("fields,msg", [
    (dict(win_range=5), b"win_range"), (dict(win_doppler=5), b"win_doppler"),
    (dict(n_doppler=2, win_doppler=1), b"n_doppler"), (dict(n_doppler=8, win_doppler=4), b"n_doppler"),
    (dict(n_doppler=65537), b"n_doppler"),
    (dict(n_range=0), b"n_range"), (dict(n_range=65537), b"n_range"),
    (dict(max_dets=0), b"max_dets"), (dict(max_dets=1 << 31), b"max_dets"),
    (dict(device_id=64), b"device_id"), (dict(device_id=-1), b"device_id"),
])
def test_plots_create_rejects_bad_config(lib_built, fields, msg):
    cfg = L.FmcwPlotsConfig()
    lib_built.fmcw_plots_config_default(C.byref(cfg))
    for k, v in fields.items():
        setattr(cfg, k, v)
    h = C.c_void_p()
    assert lib_built.fmcw_plots_create(C.byref(cfg), C.byref(h)) == L.FMCW_EINVAL
    assert msg in lib_built.fmcw_last_error()
    assert not h.value


def test_plots_null_arguments(lib_built):
    cfg = L.FmcwPlotsConfig()
    lib_built.fmcw_plots_config_default(None)            # ignored
    lib_built.fmcw_plots_config_default(C.byref(cfg))
    h = C.c_void_p()
    assert lib_built.fmcw_plots_create(None, C.byref(h)) == L.FMCW_EINVAL
    assert lib_built.fmcw_plots_create(C.byref(cfg), None) == L.FMCW_EINVAL
    assert lib_built.fmcw_plots_enqueue(None, None, 0, None, None, 0, None, None) == L.FMCW_EINVAL
    assert lib_built.fmcw_plots_destroy(None) == L.FMCW_OK


def test_plots_create_without_device(lib_built):
    if L.device_count() > 0:
        pytest.skip("a device is present; covered by the GPU tests")
    cfg = L.FmcwPlotsConfig()
    lib_built.fmcw_plots_config_default(C.byref(cfg))
    h = C.c_void_p()
    assert lib_built.fmcw_plots_create(C.byref(cfg), C.byref(h)) == L.FMCW_ENODEV
    assert not h.value


def test_reference_on_two_targets():
    """The fp64 oracle with the reference 2-D OS-CFAR on two_targets 1024 x 128, seed 1234: 120
    detections, 66 of them below range 300 (so the tracker's 64 slots never see range 500); 3 x 3
    grouping leaves five plots, 9 x 9 exactly the two targets."""
    dets = O.process(synth.frame(1024, 128, 1, "two_targets", 1234), O.Cfar2D())["dets"]
    assert len(dets) == 120 and int((dets["range"] < 300).sum()) == 66
    p = plots_ref(dets, 1024, 128, 1, 1)
    assert list(zip(p["range"].tolist(), p["doppler"].tolist(), p["n_cells"].tolist())) == \
        [(94, 5, 1), (100, 5, 9), (100, 119, 1), (106, 5, 1), (500, 118, 9)]
    p = plots_ref(dets, 1024, 128, 4, 4)
    assert list(zip(p["range"].tolist(), p["doppler"].tolist(), p["n_cells"].tolist())) == \
        [(100, 5, 29), (500, 118, 29)]
    assert np.all(np.abs(p["d_range"]) <= 4) and np.all(np.abs(p["d_doppler"]) <= 4)


def test_reference_hand_cases():
    """plots_ref itself on lists small enough to check by eye."""
    from fmcw import DET_DTYPE

    def mk(rows):
        a = np.zeros(len(rows), DET_DTYPE)
        for i, (f, r, d, m) in enumerate(rows):
            a[i] = (f, r, d, m, 1.0)
        return a
    # Doppler wrap: columns 7 and 0 of an 8-wide map are neighbours; the larger wins
    p = plots_ref(mk([(0, 3, 0, 2.0), (0, 3, 7, 5.0)]), 8, 8, 1, 1)
    assert [(int(x["doppler"]), int(x["n_cells"])) for x in p] == [(7, 2)]
    assert p["d_doppler"][0] == pytest.approx(2.0 / 7.0) and p["d_range"][0] == 0
    # range is clamped: rows 0 and 7 are not neighbours; same cell in adjacent frames does not group
    p = plots_ref(mk([(0, 0, 2, 1.0), (0, 7, 2, 3.0), (1, 7, 2, 4.0)]), 8, 8, 1, 1)
    assert len(p) == 3 and list(p["n_cells"]) == [1, 1, 1]
    # a 2 x 2 plateau: the first in list order wins
    p = plots_ref(mk([(0, 2, 2, 4.0), (0, 2, 3, 4.0), (0, 3, 2, 4.0), (0, 3, 3, 4.0)]), 8, 8, 1, 1)
    assert [(int(x["range"]), int(x["doppler"]), int(x["n_cells"])) for x in p] == [(2, 2, 4)]
    assert p["d_range"][0] == 0.5 and p["d_doppler"][0] == 0.5
