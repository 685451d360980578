"""Velocity unfolding, host side (no GPU): the specification itself -- tests/unfold_ref.py on hand
cases whose answers are worked out below -- the C-ABI's layouts and argument checks (validated before
any device access), the Python wrapper's arithmetic, and the scenario's fighter through the fp64
oracle chain, plots_ref and unfold_ref.

Hand cases use the scenario's stagger unless they say otherwise: PRF units 8 / 9 / 10 (8, 9, 10 kHz,
f0 1 kHz), Nc 32, v_max 512, tolerances 1 / 1, m_of 2, one stream, 8 range bins.  The fine unit is
f0 / Nc = 31.25 Hz.  The fighter (-340.29 m/s at 0.1 m: -6805.8 Hz = -217.8 fine units) sits at
-217.8 / 8 = -27.2 -> bin 5, -217.8 / 9 = -24.2 -> bin 8 and -217.8 / 10 = -21.8 -> bin 10.
"""
import ctypes as C
import functools
import subprocess

import numpy as np
import pytest

import scenario_ref as S
from fmcw import DET_DTYPE, MPLOT_DTYPE, PLOT_DTYPE, VPLOT_DTYPE, VelocityUnfolder, synth, velocity_mps
from fmcw import _lib as L
from tile_edge import TILE_EDGE_SIZES
from unfold_ref import (F0_HZ, FIGHTER_FACT, TILE_EDGE_CFG, TRUTH_MPS, Cfg, VPLOT_REF_DTYPE, fighter_fact, hypotheses, n_dwells,
                        out_doppler, predicted_bin, records, scenario_cfg, signed_bin, tile_edge_list, truth_fine,
                        unfold_ref)

NEW_SYMBOLS = ("fmcw_unfold_config_default", "fmcw_unfold_create", "fmcw_unfold_destroy", "fmcw_unfold_enqueue",
               "fmcw_unfold_set_grid_for_test")
FIELDS = ["n_range", "n_doppler", "n_prf", "prf_units", "prf_phase", "step", "zero_bin", "v_max", "out_unit",
          "tol_range", "tol_doppler", "m_of", "n_streams", "max_recs", "max_frames", "device_id"]
ONE = C.c_void_p(0x1000)   # a non-null, aligned stand-in: the checks below never dereference it
SHOW = ("frame", "range", "doppler", "v_fine", "fold", "n_hits", "hit_mask", "pos", "n_ties", "src")


def hand(rows, n_scans, **kw):
    """unfold_ref on (frame, range, doppler, mag) rows under the hand cases' configuration: (a tuple of
    SHOW per report, sum_mag per report, status words 2 and 3)."""
    base = dict(n_range=8, n_doppler=32, v_max=512, step=3)
    base.update(kw)
    out, beyond, tied = unfold_ref(records(rows, DET_DTYPE), n_scans, Cfg(**base))
    return [tuple(int(p[k]) for k in SHOW) for p in out], [float(x) for x in out["sum_mag"]], (beyond, tied)


# ---- the pieces ------------------------------------------------------------------------------
def test_arithmetic_of_the_specification():
    assert [signed_bin(d, 0, 32) for d in (0, 15, 16, 31)] == [0, 15, -16, -1]
    assert [signed_bin(d, 0, 9) for d in (4, 5, 8)] == [4, -4, -1]                  # odd Nc: (Nc + 1) / 2 = 5
    assert [signed_bin(d, 16, 32) for d in (16, 21, 0, 15)] == [0, 5, -16, -1]
    # ds 5 at 8 units, v_max 512: |5 + 32 m| <= 64 gives m = -2 .. 1
    assert hypotheses(5, 32, 8, 512) == [(-2, -472), (-1, -216), (0, 40), (1, 296)]
    assert hypotheses(5, 32, 8, 39) == [] and hypotheses(0, 32, 8, 0) == [(0, 0)]
    assert len(hypotheses(0, 32, 8, 32 * 32 * 8)) == 65                             # the most there can be
    # floor((2 v + p) / (2 p)): halves go up, also below zero
    assert [predicted_bin(v, 8, 0, 32) for v in (-216, -220, -212, 4, 3, -4, -5)] == [5, 5, 6, 1, 0, 0, 31]
    assert predicted_bin(-216, 9, 16, 32) == 24 and predicted_bin(-216, 10, 16, 32) == 26
    assert [out_doppler(v, 512, 8) for v in (-512, -216, 0, 512)] == [0, 37, 64, 128]
    assert [n_dwells(n, 3, 1) for n in (2, 3, 9)] == [0, 1, 7] and [n_dwells(n, 3, 3) for n in (3, 5, 6, 9)] == [1, 1, 2, 3]


# ---- hand cases ------------------------------------------------------------------------------
def test_the_fighter():
    """Bins 5, 8, 10.  The 8 kHz record: ds 5, hypotheses -472, -216, 40, 296.  v = -216 predicts
    floor(-432 + 9, 18) = -24 -> bin 8 at 9 kHz and floor(-432 + 10, 20) = -22 -> bin 10 at 10 kHz: both
    there, 3 hits, mask 0b111, fold -1; the others predict 9 kHz bins 12 (-472), 4 (40), 1 (296): nothing
    within one bin.  The 9 kHz record: (8 - 32) 9 = -216 predicts bin 5 at 8 kHz, a hit before its own
    position, so it does not report; nor does the 10 kHz one ((10 - 32) 10 = -220 -> -27.5 -> bin 5).
    .doppler = floor((2 (-216 + 512) + 8) / 16) = 37; sum_mag = 3 + 2 + 4."""
    got, sums, st = hand([(0, 3, 5, 3.0), (1, 3, 8, 2.0), (2, 3, 10, 4.0)], 3)
    assert got == [(0, 3, 37, -216, -1, 3, 0b111, 0, 1, 0)] and sums == [9.0] and st == (0, 0)


def test_shifted_bins_of_the_testbench():
    """tb_tactical adds Nc / 2 to its bins: 21 / 24 / 26 with zero_bin 16 is the same target."""
    got, _, _ = hand([(0, 3, 21, 3.0), (1, 3, 24, 2.0), (2, 3, 26, 4.0)], 3, zero_bin=16)
    assert got == [(0, 3, 37, -216, -1, 3, 0b111, 0, 1, 0)]


def test_blind_at_one_prf_and_an_empty_scan():
    """The 9 kHz scan holds no record at all (an empty scan inside the dwell): the 8 kHz record still
    finds bin 10 at 10 kHz, 2 of 3, mask 0b101.  Blind at 8 kHz instead: the 9 kHz record is the first
    to see the target, (8 - 32) 9 = -216 finds nothing at 8 kHz and bin 10 at 10 kHz; it owns the
    report at position 1 with mask 0b110 (its other hypotheses -504, 72, 360 predict bins 14, 7, 4)."""
    got, sums, _ = hand([(0, 3, 5, 5.0), (2, 3, 10, 3.0)], 3)
    assert got == [(0, 3, 37, -216, -1, 2, 0b101, 0, 1, 0)] and sums == [8.0]
    got, sums, _ = hand([(1, 3, 8, 5.0), (2, 3, 10, 3.0)], 3)
    assert got == [(0, 3, 37, -216, -1, 2, 0b110, 1, 1, 0)] and sums == [8.0]
    # with all three hits required neither reports
    assert hand([(1, 3, 8, 5.0), (2, 3, 10, 3.0)], 3, m_of=3)[0] == []


def test_predicted_bin_wraps_through_the_last_bin():
    """v = 0 predicts bin 0 everywhere; the records at bin 31 (9 kHz) and bin 1 (10 kHz) are within one
    bin of it across the wrap.  The 9 kHz record itself (ds -1, v = -9 -> 8 kHz bin floor(-18 + 8, 16) =
    -1 -> 31, window 30 .. 0) sees the first record at an earlier position."""
    got, sums, _ = hand([(0, 3, 0, 5.0), (1, 3, 31, 4.0), (2, 3, 1, 3.0)], 3)
    assert got == [(0, 3, 64, 0, 0, 3, 0b111, 0, 1, 0)] and sums == [12.0]
    # one bin further away it is a hit no longer
    got, _, _ = hand([(0, 3, 0, 5.0), (1, 3, 30, 4.0), (2, 3, 1, 3.0)], 3)
    assert got[0][5:7] == (2, 0b101)


def test_range_window_is_clamped():
    """Range row 0 has no row -1 and row 7 of 8 no row 8: the record at row 0 finds its partner in row 1,
    the one at row 7 its partners in rows 6 and 7, and nothing else is found."""
    got, sums, _ = hand([(0, 0, 5, 5.0), (1, 1, 8, 4.0), (0, 7, 5, 5.0), (1, 6, 8, 4.0), (2, 7, 10, 2.0)], 3)
    assert got == [(0, 0, 37, -216, -1, 2, 0b011, 0, 1, 0), (0, 7, 37, -216, -1, 3, 0b111, 0, 1, 1)]
    assert sums == [9.0, 11.0]
    # tol_range 0: the partners in the neighbouring rows are gone
    got, _, _ = hand([(0, 0, 5, 5.0), (1, 1, 8, 4.0), (0, 7, 5, 5.0), (1, 6, 8, 4.0), (2, 7, 10, 2.0)], 3, tol_range=0)
    assert got == [(0, 7, 37, -216, -1, 2, 0b101, 0, 1, 1)]


def test_two_targets_in_one_range_bin():
    """The fighter (5, 8, 10) and a second target at v = 120 (bins 15, 13, 12) share range bin 3.  Each
    record reports at most once, for its best hypothesis, and all six records belong to a 3-hit
    hypothesis whose first hit is the 8 kHz scan: two reports, no ghost, with tolerance 1 and with 0."""
    rows = [(0, 3, 5, 5.0), (0, 3, 15, 4.0), (1, 3, 8, 5.0), (1, 3, 13, 4.0), (2, 3, 10, 5.0), (2, 3, 12, 4.0)]
    for tol in (1, 0):
        got, sums, st = hand(rows, 3, tol_range=tol, tol_doppler=tol)
        assert got == [(0, 3, 37, -216, -1, 3, 7, 0, 1, 0), (0, 3, 79, 120, 0, 3, 7, 0, 1, 1)]
        assert sums == [15.0, 12.0] and st == (0, 0)


def test_v_max_zero():
    """Only v = 0 exists: a record reports only from the zero bin; (4, 1) has no hypothesis at all."""
    got, sums, _ = hand([(0, 3, 0, 5.0), (0, 4, 1, 5.0), (1, 3, 0, 4.0), (2, 3, 31, 3.0)], 3, v_max=0)
    assert got == [(0, 3, 0, 0, 0, 3, 7, 0, 1, 0)] and sums == [12.0]


def test_m_of_one():
    """Every record whose best hypothesis has no earlier hit reports: the lone record at 9 kHz bin 20 (ds
    -12, hypotheses -396, -108, 180, 468, one hit each: 4 ties, the slowest wins) reports too, and is
    counted in the tied word."""
    got, sums, st = hand([(0, 3, 5, 5.0), (1, 3, 8, 4.0), (1, 6, 20, 4.0), (2, 3, 10, 3.0)], 3, m_of=1)
    assert got == [(0, 3, 37, -216, -1, 3, 7, 0, 1, 0), (0, 6, 51, -108, 0, 1, 0b010, 1, 4, 2)]
    assert sums == [12.0, 4.0] and st == (0, 1)


def test_two_and_four_prfs():
    got, sums, _ = hand([(0, 3, 5, 5.0), (1, 3, 8, 4.0)], 2, prf_units=(8, 9), step=2)
    assert got == [(0, 3, 37, -216, -1, 2, 0b11, 0, 1, 0)] and sums == [9.0]
    # 11 units: -216 / 11 = -19.6 -> -20 -> bin 12
    got, sums, _ = hand([(0, 3, 5, 5.0), (1, 3, 8, 4.0), (2, 3, 10, 3.0), (3, 3, 12, 2.0)], 4, prf_units=(8, 9, 10, 11),
                        step=4, m_of=4)
    assert got == [(0, 3, 37, -216, -1, 4, 0b1111, 0, 1, 0)] and sums == [14.0]


def test_step_one_against_step_k():
    """Six scans of the fighter.  step 3: dwells 0 and 1 (scans 0-2, 3-5).  step 1: four dwells, each owned
    by its first scan's record; the one that starts at 10 kHz reads (10 - 32) 10 = -220."""
    rows = [(s, 3, (5, 8, 10)[s % 3], 1.0 + s) for s in range(6)]
    got, sums, _ = hand(rows, 6, step=3)
    assert [(g[0], g[3], g[9]) for g in got] == [(0, -216, 0), (1, -216, 3)] and sums == [6.0, 15.0]
    got, sums, _ = hand(rows, 6, step=1)
    assert [(g[0], g[3], g[9]) for g in got] == [(0, -216, 0), (1, -216, 1), (2, -220, 2), (3, -216, 3)]
    assert sums == [6.0, 9.0, 12.0, 15.0] and all(g[5:8] == (3, 7, 0) for g in got)
    # prf_phase 1: scan 0 is the 9 kHz scan, so no velocity explains all three bins of a dwell
    assert all(g[5] < 3 for g in hand(rows, 6, step=3, prf_phase=1)[0])


def test_largest_record_of_the_window_is_the_hit():
    """Three records in the 9 kHz window of bin 8: the hit's record is the largest, so sum_mag is 5 + 3;
    with equal magnitudes the first in list order is taken (same sum either way: 5 + 2)."""
    got, sums, _ = hand([(0, 3, 5, 5.0), (1, 2, 8, 2.0), (1, 3, 7, 3.0), (1, 4, 9, 1.0)], 3)
    assert got == [(0, 3, 37, -216, -1, 2, 0b011, 0, 1, 0)] and sums == [8.0]
    got, sums, _ = hand([(0, 3, 5, 5.0), (1, 2, 8, 2.0), (1, 3, 7, 2.0), (1, 4, 9, 1.0)], 3)
    assert got == [(0, 3, 37, -216, -1, 2, 0b011, 0, 1, 0)] and sums == [7.0]


def test_streams_never_interact_and_order():
    """Two streams: frame m is scan m // 2 of stream m % 2.  Stream 0 holds the fighter, stream 1 only its
    9 kHz and 10 kHz records.  Reports come by (dwell, stream), so .frame never decreases, and the
    records beyond n_scans are counted and ignored."""
    rows = [(0, 3, 5, 5.0), (2, 3, 8, 4.0), (4, 3, 10, 3.0), (3, 3, 8, 4.0), (5, 3, 10, 3.0), (6, 3, 5, 1.0), (7, 3, 5, 1.0)]
    got, _, st = hand(rows, 3, n_streams=2)
    assert got == [(0, 3, 37, -216, -1, 3, 7, 0, 1, 0), (1, 3, 37, -216, -1, 2, 6, 1, 1, 2)] and st == (2, 0)


# ---- layout and validation ---------------------------------------------------------------------
@pytest.mark.parametrize("n", TILE_EDGE_SIZES)
def test_tile_edge_lists_have_reports(n):
    want, beyond, _ = unfold_ref(tile_edge_list(n), 6, TILE_EDGE_CFG)
    assert beyond == 0 and len(want) > 0


def default_cfg(lib):
    cfg = L.FmcwUnfoldConfig()
    lib.fmcw_unfold_config_default(C.byref(cfg))
    return cfg


def test_layouts_defaults_and_abi(lib_built):
    assert C.sizeof(L.FmcwVplot) == 32 and C.sizeof(L.FmcwUnfoldConfig) == 92
    offs = {n: getattr(L.FmcwVplot, n).offset for n, _ in L.FmcwVplot._fields_}
    assert offs == {"frame": 0, "range": 4, "doppler": 6, "mag": 8, "v_fine": 12, "fold": 16, "n_hits": 18,
                    "hit_mask": 19, "sum_mag": 20, "pos": 24, "n_ties": 26, "src": 28}
    for dt in (VPLOT_DTYPE, VPLOT_REF_DTYPE):
        assert dt.itemsize == 32 and {n: dt.fields[n][1] for n in dt.names} == offs
    types = {n: t for n, t in L.FmcwVplot._fields_}
    assert types["v_fine"] is C.c_int32 and types["fold"] is C.c_int16 and types["n_hits"] is C.c_uint8
    # the tracker reads frame / range / doppler / mag where fmcw_plot and fmcw_mplot have them
    for n in ("frame", "range", "doppler", "mag"):
        assert VPLOT_DTYPE.fields[n] == PLOT_DTYPE.fields[n] == MPLOT_DTYPE.fields[n]
    assert [f[0] for f in L.FmcwUnfoldConfig._fields_] == FIELDS
    want = [0, 4, 8, 12] + list(range(44, 92, 4))
    assert [getattr(L.FmcwUnfoldConfig, n).offset for n in FIELDS] == want
    src = L.HEADER_PATH.read_text()
    body = src[src.index("typedef struct fmcw_unfold_config {"):src.index("} fmcw_unfold_config;")]
    assert sorted(FIELDS, key=lambda n: body.index(f"_t {n}")) == FIELDS   # the declarations
    assert "#define FMCW_UNFOLD_STATUS_WORDS 4" in src and L.UNFOLD_STATUS_WORDS == 4
    cfg = default_cfg(lib_built)
    got = [list(getattr(cfg, n)) if n == "prf_units" else getattr(cfg, n) for n in FIELDS]
    assert got == [1024, 128, 3, [8, 9, 10, 0, 0, 0, 0, 0], 0, 3, 0, 2 * 128 * 8, 8, 1, 1, 2, 1, 1 << 20, 1024, 0]
    assert lib_built.fmcw_abi_version() == 8 and "Still 8 with the velocity unfolder" in src


def test_new_symbols_exported(lib_built):
    out = subprocess.run(["nm", "-D", "--defined-only", str(L.LIB_PATH)], capture_output=True, text=True,
                         check=True).stdout
    src = L.HEADER_PATH.read_text()
    for name in NEW_SYMBOLS:
        assert f" T {name}\n" in out, name
        assert name in L.SIGNATURES and f"{name}(" in src


@pytest.mark.parametrize("fields,msg", [
    (dict(n_range=0), b"n_range"), (dict(n_range=65537), b"n_range"),
    (dict(n_doppler=2), b"n_doppler"), (dict(n_doppler=8, tol_doppler=4, v_max=0), b"n_doppler"),
    (dict(n_doppler=65537), b"n_doppler"),
    (dict(n_prf=1), b"n_prf"), (dict(n_prf=9), b"n_prf"),
    (dict(prf_units=(0, 9, 10)), b"prf_units[0]"), (dict(prf_units=(8, 4097, 10)), b"prf_units[1]"),
    (dict(prf_units=(8, 9, 8)), b"prf_units[0] and prf_units[2]"), (dict(n_prf=4), b"prf_units[3]"),
    (dict(prf_phase=3), b"prf_phase"), (dict(step=0), b"step"), (dict(step=4), b"step"),
    (dict(zero_bin=128), b"zero_bin"),
    (dict(v_max=32 * 128 * 8 + 1, out_unit=64), b"v_max"), (dict(prf_units=(8, 9, 4), v_max=32 * 128 * 4 + 1), b"v_max"),
    (dict(out_unit=0), b"out_unit"), (dict(out_unit=65536), b"out_unit"),
    (dict(v_max=32767, out_unit=1), None), (dict(v_max=32768, out_unit=1), b"out_unit"),   # 65535 / 65537 output bins
    (dict(tol_range=5), b"tol_range"), (dict(tol_doppler=5), b"tol_doppler"),
    (dict(m_of=0), b"m_of"), (dict(m_of=4), b"m_of"),
    (dict(n_streams=0), b"n_streams"), (dict(n_streams=4097, max_frames=4097), b"n_streams"),
    (dict(max_recs=0), b"max_recs"), (dict(max_recs=1 << 31), b"max_recs"),
    (dict(max_recs=1 << 30, step=1), b"max_recs"),   # 3 dwells per record
    (dict(max_frames=0), b"max_frames"), (dict(n_streams=3, max_frames=1024), b"max_frames"),
    (dict(n_streams=8, max_frames=4), b"max_frames"), (dict(max_frames=1 << 30), b"max_frames"),
    (dict(device_id=64), b"device_id"), (dict(device_id=-1), b"device_id"),
])
def test_create_checks_every_field(lib_built, fields, msg):
    """Each limit is FMCW_EINVAL naming the field, before any device access; a configuration at the
    limit (msg None) passes validation and, without a device, stops at FMCW_ENODEV."""
    cfg = default_cfg(lib_built)
    for k, v in fields.items():
        if k == "prf_units":
            for i, p in enumerate(v):
                cfg.prf_units[i] = p
        else:
            setattr(cfg, k, v)
    h = C.c_void_p(1)
    rc = lib_built.fmcw_unfold_create(C.byref(cfg), C.byref(h))
    if msg is None:
        # (with a device the large scratch may not fit: FMCW_ENOMEM is not a validation error either)
        assert rc in ((L.FMCW_ENODEV,) if L.device_count() < 1 else (L.FMCW_OK, L.FMCW_ENOMEM)), lib_built.fmcw_last_error()
        if rc == L.FMCW_OK:
            assert lib_built.fmcw_unfold_destroy(h) == L.FMCW_OK
        return
    assert rc == L.FMCW_EINVAL
    assert msg in lib_built.fmcw_last_error(), lib_built.fmcw_last_error()
    assert not h.value


def test_null_arguments(lib_built):
    lib = lib_built
    lib.fmcw_unfold_config_default(None)            # ignored
    cfg = default_cfg(lib)
    h = C.c_void_p()
    assert lib.fmcw_unfold_create(None, C.byref(h)) == L.FMCW_EINVAL
    assert lib.fmcw_unfold_create(C.byref(cfg), None) == L.FMCW_EINVAL
    assert lib.fmcw_unfold_destroy(None) == L.FMCW_OK
    assert lib.fmcw_unfold_set_grid_for_test(None, 1) == L.FMCW_EINVAL and lib.fmcw_last_error() == b"null unfolder"


@pytest.mark.parametrize("kw,msg", [
    (dict(rec_stride=8), b"rec_stride"), (dict(rec_stride=24), b"rec_stride"), (dict(rec_stride=0), b"rec_stride"),
    (dict(recs=None), b"recs_dev"), (dict(n_recs=None), b"n_recs_dev"), (dict(out=None), b"out_dev"),
    (dict(status=None), b"status_dev"),
    (dict(out=C.c_void_p(0x1008)), b"out_dev must be 16-byte aligned"),
    (dict(recs=C.c_void_p(0x1004)), b"recs_dev must be 16-byte aligned"),
    (dict(), b"null unfolder"),
])
def test_enqueue_checks_arguments_before_the_unfolder(lib_built, kw, msg):
    a = dict(recs=ONE, rec_stride=16, rec_cap=4, n_recs=ONE, n_scans=3, out=ONE, out_cap=4, status=ONE)
    a.update(kw)
    rc = lib_built.fmcw_unfold_enqueue(None, a["recs"], a["rec_stride"], a["rec_cap"], a["n_recs"], a["n_scans"],
                                       a["out"], a["out_cap"], a["status"], None)
    assert rc == L.FMCW_EINVAL
    assert msg in lib_built.fmcw_last_error(), lib_built.fmcw_last_error()


def test_create_without_device_and_n_scans_limit(lib_built):
    """Without a device a valid configuration is FMCW_ENODEV; with one, n_scans * n_streams above
    max_frames is FMCW_EINVAL naming n_scans before anything is launched."""
    cfg = default_cfg(lib_built)
    cfg.n_streams, cfg.max_frames = 2, 6
    h = C.c_void_p(1)
    rc = lib_built.fmcw_unfold_create(C.byref(cfg), C.byref(h))
    if L.device_count() < 1:
        assert rc == L.FMCW_ENODEV and not h.value
        return
    assert rc == L.FMCW_OK and h.value
    try:
        assert lib_built.fmcw_unfold_enqueue(h, ONE, 16, 4, ONE, 4, ONE, 4, ONE, None) == L.FMCW_EINVAL
        assert b"n_scans" in lib_built.fmcw_last_error() and b"max_frames" in lib_built.fmcw_last_error()
    finally:
        assert lib_built.fmcw_unfold_destroy(h) == L.FMCW_OK


def test_python_class(lib_built):
    assert VelocityUnfolder.__init__.__defaults__ == (1024, 128, (8, 9, 10), 0, None, 0, None, None, (1, 1), 2, 1,
                                                      1 << 20, None, 0)
    for name in ("enqueue", "unfold", "from_physical", "n_dwells", "set_grid_for_test", "close"):
        assert callable(getattr(VelocityUnfolder, name))
    with pytest.raises(L.FmcwError, match="tol_doppler"):
        VelocityUnfolder(64, 32, tol=(1, 5))
    with pytest.raises(ValueError, match="4096"):
        VelocityUnfolder.from_physical((8000.0, 8001.0, 9000.0), 0.1, 400.0, 32)      # f0 1 Hz: units 8000 ..
    with pytest.raises(ValueError, match="4096"):
        VelocityUnfolder.from_physical((8000.0, 8000.5), 0.1, 400.0, 32)              # f0 0.5 Hz
    # 8 / 9 / 10 kHz: f0 1 kHz; 12.5 / 15 kHz: f0 2.5 kHz, units 5 / 6.  Creation then stops at the device.
    try:
        with VelocityUnfolder.from_physical(synth.TAC_PRF_HZ, synth.TAC_WAVELENGTH, 500.0, 32, N_RANGE=128) as u:
            assert list(u.cfg.prf_units)[:3] == [8, 9, 10] and u.f0_hz == 1000.0 and u.cfg.v_max == 320
            assert u.cfg.out_unit == 8 and u.cfg.step == 3 and u.n_dwells(9) == 3
    except L.FmcwError as e:
        assert e.code == L.FMCW_ENODEV and L.device_count() < 1
    p = np.zeros(2, VPLOT_DTYPE)
    p["v_fine"] = [-216, 320]
    # -216 fine units of 1000 / 32 Hz = -6750 Hz; times 0.05 m
    np.testing.assert_allclose(velocity_mps(p, 1000.0, 32, 0.1), [-337.5, 500.0])


# ---- the scenario's fighter, on the CPU ----------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_vplots(scene_id):
    scene = S.BY_ID[scene_id]
    plots = S.oracle_plots(scene, S.reference(scene, 2, "float").dets)
    out, beyond, _ = unfold_ref(plots, scene.n_scans, scenario_cfg(scene))
    assert beyond == 0
    return plots, out


@pytest.mark.parametrize("scene_id", sorted(FIGHTER_FACT))
def test_scenario_fighter_through_the_references(scene_id):
    """The fp64 oracle chain behind the 2-pulse canceller -> plots_ref -> unfold_ref, K 3, step 1.

    Two dwells qualify in each scene: 0 (scans 0-2) and 6 (scans 6-8); the notch takes scans 3-5.
    sea-128x32: the fact holds in both (v_fine -216 against -217.8).
    sea-256x64: it holds in dwell 0 (v_fine -432 against -435.6) and NOT in dwell 6.  The claim is narrowed
    there to what the oracle supports: at 256 x 64 the strong targets' Doppler sidelobes cross the CFAR, so
    the fighter's range row holds further plots; in dwell 6 some lie within one bin of where v = 80 (fold 0
    of the same bin 10) folds to at 9 and 10 kHz.  Both hypotheses collect 3 hits, the report says so
    (n_ties 2), and rule 8 gives the slower one.  The specification stays as it is; the test pins the
    tie."""
    scene = S.BY_ID[scene_id]
    plots, out = oracle_vplots(scene_id)
    qualifying, holds, reports = fighter_fact(scene, plots, out)
    print(f"{scene_id}: {len(plots)} plots, {len(out)} reports, qualifying dwells {qualifying}, fact holds in {holds}; "
          f"truth {truth_fine(scene):.1f}, reports {[(j, int(r['v_fine']), int(r['n_hits']), int(r['n_ties'])) for j, r in reports.items()]}")
    assert len(qualifying) > 0
    assert (qualifying, holds) == FIGHTER_FACT[scene_id]
    for j in qualifying:
        assert int(reports[j]["n_hits"]) == 3 and int(reports[j]["hit_mask"]) == 7
        assert j in holds or int(reports[j]["n_ties"]) > 1       # a wrong velocity is never reported as unique
    if scene_id == "sea-256x64":
        assert (int(reports[6]["v_fine"]), int(reports[6]["fold"]), int(reports[6]["n_ties"])) == (80, 0, 2)
    # the unfolded velocity in m/s, within one output bin (8 x 31.25 Hz x 0.05 m = 12.5 m/s at Nc 32)
    v = velocity_mps(np.array([reports[j] for j in holds]), F0_HZ, scene.nc, synth.TAC_WAVELENGTH)
    assert np.all(np.abs(v - TRUTH_MPS) <= 8 * F0_HZ / scene.nc * synth.TAC_WAVELENGTH / 2)
