"""The device tracker without a GPU: the C-ABI's layout, defaults, exports and argument checks (they
come before any device access), the reference helper tests/tws_dev_ref.py against a hand-written
case, and formats.write_tracks over the host tracker's and the device tracker's result shapes."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from fmcw import _lib as L
from fmcw import DET_DTYPE, PLOT_DTYPE, TRACK_DTYPE, DeviceTwsTracker, cli, formats
import tws_dev_ref as R

NEW_SYMBOLS = ("fmcw_tws_dev_config_default", "fmcw_tws_dev_create", "fmcw_tws_dev_destroy", "fmcw_tws_dev_reset",
               "fmcw_tws_dev_enqueue", "fmcw_tws_dev_set_grid_for_test")
ONE = C.c_void_p(0x1000)   # a non-null, aligned stand-in: the checks below never dereference it


def default_cfg(lib):
    cfg = L.FmcwTwsDevConfig()
    lib.fmcw_tws_dev_config_default(C.byref(cfg))
    return cfg


def test_layout_and_defaults(lib_built):
    assert C.sizeof(L.FmcwTwsConfig) == 36 and C.sizeof(L.FmcwTwsDevConfig) == 48 and C.sizeof(L.FmcwTrack) == 28
    assert [f[0] for f in L.FmcwTwsDevConfig._fields_] == ["tws", "n_streams", "max_scans", "device_id"]
    assert (L.FmcwTwsDevConfig.tws.offset, L.FmcwTwsDevConfig.n_streams.offset, L.FmcwTwsDevConfig.max_scans.offset,
            L.FmcwTwsDevConfig.device_id.offset) == (0, 36, 40, 44)
    src = L.HEADER_PATH.read_text()
    body = src[src.index("typedef struct fmcw_tws_dev_config {"):src.index("} fmcw_tws_dev_config;")]
    decl = ["fmcw_tws_config tws;", "uint32_t n_streams;", "uint32_t max_scans;", "int32_t device_id;"]
    assert all(d in body for d in decl) and sorted(decl, key=body.index) == decl
    assert f"#define FMCW_TWS_DEV_STATUS_WORDS {L.TWS_DEV_STATUS_WORDS}" in src
    cfg, host = default_cfg(lib_built), L.FmcwTwsConfig()
    lib_built.fmcw_tws_config_default(C.byref(host))
    assert bytes(cfg.tws) == bytes(host)
    assert (cfg.tws.max_tracks, cfg.tws.max_dets, cfg.tws.rtl_compat) == (32, 64, 0)
    assert (cfg.n_streams, cfg.max_scans, cfg.device_id) == (1, 1024, 0)
    assert lib_built.fmcw_abi_version() == 8 and "Still 8 with the device tracker" in src
    for dt, f in ((DET_DTYPE, L.FmcwDet), (PLOT_DTYPE, L.FmcwPlot), (TRACK_DTYPE, L.FmcwTrack)):
        assert dt.itemsize == C.sizeof(f)
        for name in dt.names:
            assert dt.fields[name][1] == getattr(f, name).offset


def test_new_symbols_exported(lib_built):
    out = subprocess.run(["nm", "-D", "--defined-only", str(L.LIB_PATH)], capture_output=True, text=True,
                         check=True).stdout
    src = L.HEADER_PATH.read_text()
    for name in NEW_SYMBOLS:
        assert f" T {name}\n" in out, name
        assert name in L.SIGNATURES and f"{name}(" in src


@pytest.mark.parametrize("field,value,msg", [
    ("tws.max_tracks", 0, b"max_tracks"), ("tws.max_tracks", 65, b"max_tracks"),
    ("tws.max_dets", 0, b"max_dets"), ("tws.max_dets", 65, b"max_dets"),
    ("tws.alpha_q8", 256, b"alpha_q8"), ("tws.beta_q8", 256, b"beta_q8"),
    ("tws.gate_r", 4097, b"gate_r"), ("tws.gate_d", 4097, b"gate_d"),
    ("n_streams", 0, b"n_streams"), ("n_streams", 4097, b"n_streams"),
    ("max_scans", 0, b"max_scans"), ("max_scans", 1 << 31, b"max_scans"),
    ("device_id", -1, b"device_id"), ("device_id", 64, b"device_id"),
])
def test_create_rejects_bad_fields(lib_built, field, value, msg):
    cfg = default_cfg(lib_built)
    obj = cfg
    *path, leaf = field.split(".")
    for p in path:
        obj = getattr(obj, p)
    setattr(obj, leaf, value)
    h = C.c_void_p(1)
    assert lib_built.fmcw_tws_dev_create(C.byref(cfg), C.byref(h)) == L.FMCW_EINVAL
    assert msg in lib_built.fmcw_last_error(), lib_built.fmcw_last_error()
    assert not h.value


def test_python_class_rejects_bad_generics(lib_built):
    from fmcw import FmcwError
    for kw in (dict(MAX_TRACKS=0), dict(MAX_DETS=65), dict(ALPHA_GAIN=256), dict(n_streams=0), dict(max_scans=0)):
        with pytest.raises(FmcwError):
            DeviceTwsTracker(**kw)


def test_null_arguments(lib_built):
    lib = lib_built
    assert lib.fmcw_tws_dev_create(None, None) == L.FMCW_EINVAL
    cfg = default_cfg(lib)
    assert lib.fmcw_tws_dev_create(C.byref(cfg), None) == L.FMCW_EINVAL
    assert lib.fmcw_tws_dev_destroy(None) == L.FMCW_OK
    assert lib.fmcw_tws_dev_reset(None, None) == L.FMCW_EINVAL and b"tracker" in lib.fmcw_last_error()
    assert lib.fmcw_tws_dev_set_grid_for_test(None, 1) == L.FMCW_EINVAL and b"tracker" in lib.fmcw_last_error()
    lib.fmcw_tws_dev_config_default(None)


@pytest.mark.parametrize("kw,msg", [
    (dict(rec_stride=8), b"rec_stride"), (dict(rec_stride=24), b"rec_stride"), (dict(rec_stride=0), b"rec_stride"),
    (dict(track_cap=0), b"track_cap"),
    (dict(recs=None), b"recs_dev"), (dict(n_recs=None), b"n_recs_dev"), (dict(tracks=None), b"tracks_dev"),
    (dict(counts=None), b"counts_dev"), (dict(status=None), b"status_dev"),
    (dict(), b"null tracker"),
])
def test_enqueue_checks_arguments_before_the_tracker(lib_built, kw, msg):
    """Everything that does not depend on the tracker is checked first, so these hold with a null
    tracker on a machine without a device."""
    a = dict(recs=ONE, rec_stride=16, rec_cap=4, n_recs=ONE, n_scans=2, tracks=ONE, track_cap=4, counts=ONE,
             status=ONE)
    a.update(kw)
    rc = lib_built.fmcw_tws_dev_enqueue(None, a["recs"], a["rec_stride"], a["rec_cap"], a["n_recs"], a["n_scans"],
                                        a["tracks"], a["track_cap"], a["counts"], a["status"], None)
    assert rc == L.FMCW_EINVAL
    assert msg in lib_built.fmcw_last_error(), lib_built.fmcw_last_error()


def test_create_without_device_and_n_scans_limit(lib_built):
    """Without a device a valid configuration is FMCW_ENODEV; with one, n_scans > max_scans is
    FMCW_EINVAL naming n_scans before anything is launched (the pointers are never dereferenced)."""
    cfg = default_cfg(lib_built)
    cfg.max_scans = 4
    h = C.c_void_p(1)
    rc = lib_built.fmcw_tws_dev_create(C.byref(cfg), C.byref(h))
    if L.device_count() < 1:
        assert rc == L.FMCW_ENODEV and not h.value
        return
    assert rc == L.FMCW_OK and h.value
    try:
        assert lib_built.fmcw_tws_dev_enqueue(h, ONE, 16, 4, ONE, 5, ONE, 4, ONE, ONE, None) == L.FMCW_EINVAL
        assert b"n_scans" in lib_built.fmcw_last_error() and b"max_scans" in lib_built.fmcw_last_error()
    finally:
        assert lib_built.fmcw_tws_dev_destroy(h) == L.FMCW_OK


def mk(rows, dtype=DET_DTYPE):
    a = np.zeros(len(rows), dtype)
    for i, (f, r, d, m) in enumerate(rows):
        a[i]["frame"], a[i]["range"], a[i]["doppler"], a[i]["mag"] = f, r, d, m
    return a


def test_round_mag():
    assert [R.round_mag(m) for m in (0, -1, 0.5, 0.49, 131071.5, 131072, 3.9e9, 4.0e9, 5e9)] == \
        [0, 0, 1, 0, 131072, 131072, 3900000000, 0xFFFFFFFF, 0xFFFFFFFF]


@pytest.mark.parametrize("rtl", [False, True])
def test_reference_helper_hand_case(rtl):
    """Two streams, three scans, written out by hand.  Stream 0 sees one target at (100, 40) in every
    scan, moving one range bin per scan; stream 1 sees a target only in scan 0 (its frames 3 and 5 are
    empty).  INIT_HITS 2: TENT after scan 0 (hit 1) and after scan 1 (the promotion reads hit = 1 < 2),
    FIRM from scan 2 (hit = 2 >= 2).  alpha = 128 / 256, beta = 64 / 256.
      scan 1: predicted 400 + 0, innovation 404 - 400 = 4: pos 402, vel 1, quality 2, age 1
      scan 2: predicted 403, innovation 408 - 403 = 5: pos 403 + (5 * 128 >> 8 = 2) = 405,
              vel 1 + (5 * 64 >> 8 = 1) = 2, quality 3, age 2, reported FIRM
    One record at frame 6 (= n_scans x n_streams) is out of range, and one lies beyond rec_cap."""
    rows = [(0, 100, 40, 500.4), (1, 300, 9, 77.0), (2, 101, 40, 600.5), (4, 102, 40, 700.0), (6, 5, 5, 1.0),
            (6, 6, 6, 1.0)]
    recs = mk(rows)
    oracles = R.make_oracles(2, rtl)
    out, status = R.run_ref(recs, 3, 2, oracles, rec_cap=5)
    assert status == [1, 1]
    shape = [[(len(t), a) for t, a in row] for row in out]
    t1 = oracles[1].tracks[0]
    if rtl:
        # the RTL compares scan 2's distance 5 against the best_distance scan 1 left (4): no hit, the
        # track misses and the detection starts a second track; nothing is firm yet
        assert shape == [[(0, 1), (0, 1)], [(0, 1), (0, 1)], [(0, 2), (0, 1)]]
        t0 = oracles[0].tracks
        assert (t0[0].status, t0[0].miss, t0[0].range_pos, t0[1].status, t0[1].range_pos) == (1, 1, 403, 1, 408)
        assert oracles[0].best_distance == 0xFFFF and oracles[1].best_distance == 0xFFFF
    else:
        assert shape == [[(0, 1), (0, 1)], [(0, 1), (0, 1)], [(1, 1), (0, 1)]]
        assert out[2][0][0] == [dict(id=0, status=2, quality=3, range_q2=405, doppler_q2=160, vel_r=2, vel_d=0,
                                     last_mag=700, age=2)]
    want0 = [dict(id=0, status=2, quality=3, range_q2=405, doppler_q2=160, vel_r=2, vel_d=0, last_mag=700, age=2)]
    assert (t1.active, t1.status, t1.miss, t1.last_mag, t1.range_pos) == (True, 1, 2, 77, 1200)
    got = np.zeros(1, TRACK_DTYPE)
    got[0] = (0, 2, 3, 405, 160, 2, 0, 700, 2)
    assert R.tracks_equal(got, want0)
    got["age"] = 3
    assert not R.tracks_equal(got, want0) and not R.tracks_equal(got[:0], want0)
    # one stream: a frame is a scan, and the helper is the oracle fed frame by frame
    o1, plain = R.make_oracles(1, rtl), R.make_oracles(1, rtl)[0]
    out1, st1 = R.run_ref(recs, 7, 1, o1)
    for f in range(7):
        want = plain.scan([(r, d, R.round_mag(m)) for ff, r, d, m in rows if ff == f])
        assert out1[f][0] == want
    assert st1 == [0, 0]


def test_write_tracks_takes_both_result_shapes(tmp_path):
    """TwsTracker.scan gives (tracks, active) per scan, DeviceTwsTracker.run a list over streams of them
    per scan: with one stream the two shapes write the same bytes; with more, a scan's streams follow
    each other."""
    t = np.zeros(3, TRACK_DTYPE)
    t["id"], t["range_q2"], t["doppler_q2"], t["quality"] = [0, 1, 5], [405, -8, 4000], [160, -3, 7], [3, 15, 0]
    host = [(t[:2], 2), (t[:0], 0), (t, 4)]
    dev = [[h] for h in host]
    formats.write_tracks(tmp_path / "h.txt", host)
    formats.write_tracks(tmp_path / "d.txt", dev)
    text = (tmp_path / "h.txt").read_text()
    assert text == (tmp_path / "d.txt").read_text()
    assert text.splitlines()[:3] == ["TRK 0 R=405 D=160 Q=3", "TRK 1 R=-8 D=-3 Q=15", "SCAN_END ACTIVE=2"]
    formats.write_tracks(tmp_path / "two.txt", [[host[0], host[2]], [host[1], host[0]]])
    tracks, counts = formats.read_tracks(tmp_path / "two.txt")
    assert counts == [2, 4, 0, 2] and sorted(tracks) == [0, 1, 5]


def test_cli_tracker_argument():
    ap = cli.build_parser()
    assert ap.parse_args(["x.txt"]).tracker == "host"
    assert ap.parse_args(["x.txt", "--tracks", "--tracker", "gpu"]).tracker == "gpu"
    with pytest.raises(SystemExit):
        ap.parse_args(["x.txt", "--tracker", "fpga"])
