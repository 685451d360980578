"""Expected values of the device tracker (fmcw_tws_dev_*): a host record list with non-decreasing
frames, sliced into (scan, stream) groups and run through one oracle/tws_oracle.TwsOracle per stream.
TEST INFRASTRUCTURE ONLY.

Record frame m is scan m // n_streams of stream m % n_streams; a (scan, stream) without records is
still a scan; records at or beyond frame n_scans * n_streams are counted and ignored.  The float
magnitude is rounded as fmcw_tws_scan rounds it before the oracle sees it (<= 0 -> 0, >= 4e9 -> all
ones, else (uint64)(m + 0.5f) in fp32).
"""
import numpy as np

import tws_oracle as T

FIELDS = ("id", "status", "quality", "range_q2", "doppler_q2", "vel_r", "vel_d", "last_mag", "age")


def round_mag(m) -> int:
    m = np.float32(m)
    if m <= 0:
        return 0
    if m >= np.float32(4.0e9):
        return 0xFFFFFFFF
    return int(np.float32(m + np.float32(0.5)))


def make_oracles(n_streams, rtl, **params):
    return [T.TwsOracle(T.TwsParams(rtl=rtl, **params)) for _ in range(n_streams)]


def run_ref(records, n_scans, n_streams, oracles, rec_cap=None):
    """records: structured array with frame / range / doppler / mag.  Advances `oracles` (one per
    stream) by n_scans scans.  Returns (out, status): out[scan][stream] = (list of track dicts,
    active), status = [records beyond rec_cap, examined records at or beyond frame n_scans x n_streams]."""
    n = len(records) if rec_cap is None else min(len(records), rec_cap)
    rec = records[:n]
    groups = n_scans * n_streams
    frames = rec["frame"].astype(np.int64)
    assert np.all(np.diff(frames) >= 0), "the list must be ordered by frame"
    start = np.searchsorted(frames, np.arange(groups + 1), side="left")
    out = []
    for scan in range(n_scans):
        row = []
        for s in range(n_streams):
            m = scan * n_streams + s
            dets = [(int(r["range"]), int(r["doppler"]), round_mag(r["mag"])) for r in rec[start[m]:start[m + 1]]]
            row.append(oracles[s].scan(dets))
        out.append(row)
    return out, [len(records) - n, n - int(start[groups])]


def tracks_equal(got, want):
    """got: TRACK_DTYPE array; want: the oracle's list of dicts.  Every field, exactly."""
    if len(got) != len(want):
        return False
    return all(int(g[k]) == w[k] for g, w in zip(got, want) for k in FIELDS)
