"""NumPy restatement of the beam merger's specification (include/fmcw.h, fmcw_merge_*), with fp64
sums.  A helper for test_merge_host.py / test_gpu_merge.py, not a test module.

Input: a record array (any dtype with frame / range / doppler / mag, e.g. DET_DTYPE or PLOT_DTYPE)
strictly increasing in (frame, range, doppler).  Record frame m is scan f = m // n_beams, beam
b = m % n_beams.  Records with frame >= n_maps (a suffix) are ignored.  The neighbourhood of
P = (f, b, r, d) is every record (f, b + db, r + dr, (d + dd) mod n_doppler), P included, with
|db| <= win_beam, |dr| <= win_range, |dd| <= win_doppler, 0 <= r + dr < n_range, and the beam axis
clamped (beam_wrap 0) or circular (beam_wrap 1, n_beams >= 2 win_beam + 1).  P is a peak iff for every
other Q of its neighbourhood mag(P) > mag(Q), or mag(P) == mag(Q) and P precedes Q in the list.  One
merged plot per peak, in list order.
"""
import numpy as np

from fmcw import DET_DTYPE
from tile_edge import thin_to

MPLOT_REF_DTYPE = np.dtype([("frame", "<u4"), ("range", "<u2"), ("doppler", "<u2"), ("mag", "<f4"),
                            ("beam", "<u2"), ("n_merged", "<u2"), ("sum_mag", "<f8"),
                            ("d_beam", "<f8"), ("d_range", "<f8"), ("d_doppler", "<f8")])


def merge_ref(recs, n_range, n_doppler, n_beams, win, beam_wrap=False, n_maps=None):
    """(merged plots, records at or beyond frame n_maps).  win = (beam, range, doppler)."""
    wb, wr, wd = win
    assert n_doppler >= 2 * wd + 1 and (not beam_wrap or n_beams >= 2 * wb + 1)
    fr_all = recs["frame"].astype(np.int64)
    if n_maps is None:
        n_maps = (int(fr_all.max()) // n_beams + 1) * n_beams if len(recs) else 0
    assert n_maps % n_beams == 0
    n = int(np.searchsorted(fr_all, n_maps))
    assert np.all(fr_all[n:] >= n_maps)
    beyond = len(recs) - n
    recs = recs[:n]
    fr = fr_all[:n]
    rg = recs["range"].astype(np.int64)
    dp = recs["doppler"].astype(np.int64)
    mag = recs["mag"]
    key = (fr * n_range + rg) * n_doppler + dp
    assert np.all(np.diff(key) > 0), "list must be strictly increasing in (frame, range, doppler)"
    scan, beam = fr // n_beams, fr % n_beams
    idx = np.arange(n)
    peak = np.ones(n, bool)
    cnt = np.zeros(n, np.int64)
    s, sb, sr, sd = (np.zeros(n, np.float64) for _ in range(4))
    for db in range(-wb, wb + 1):
        bb = beam + db
        ok_beam = np.ones(n, bool) if beam_wrap else (bb >= 0) & (bb < n_beams)
        mm = scan * n_beams + bb % n_beams
        for dr in range(-wr, wr + 1):
            ok = ok_beam & (rg + dr >= 0) & (rg + dr < n_range)
            for dd in range(-wd, wd + 1):
                qkey = (mm * n_range + rg + dr) * n_doppler + (dp + dd) % n_doppler
                q = np.searchsorted(key, qkey)
                hit = ok & (q < n)
                hit[hit] = key[q[hit]] == qkey[hit]
                p, q = idx[hit], q[hit]
                mq = mag[q]
                cnt[p] += 1
                s[p] += mq.astype(np.float64)
                sb[p] += mq.astype(np.float64) * db
                sr[p] += mq.astype(np.float64) * dr
                sd[p] += mq.astype(np.float64) * dd
                other = q != p
                beaten = other & ((mq > mag[p]) | ((mq == mag[p]) & (q < p)))
                peak[p[beaten]] = False
    k = idx[peak]
    out = np.zeros(len(k), MPLOT_REF_DTYPE)
    out["frame"], out["beam"] = scan[k], beam[k]
    for name in ("range", "doppler", "mag"):
        out[name] = recs[name][k]
    out["n_merged"] = cnt[k]
    out["sum_mag"] = s[k]
    good = np.isfinite(s[k]) & (s[k] != 0)
    den = np.where(good, s[k], 1.0)
    out["d_beam"] = np.where(good, sb[k] / den, 0.0)
    out["d_range"] = np.where(good, sr[k] / den, 0.0)
    out["d_doppler"] = np.where(good, sd[k] / den, 0.0)
    return out, beyond


def tolerances(n_max, win):
    """(relative bound on sum_mag, absolute bounds on d_beam / d_range / d_doppler) for a case whose
    largest neighbourhood holds n_max records, all magnitudes non-negative.

    u = 2^-24 is fp32's unit roundoff.  The inputs (mag, and the integer offsets) are exact in both
    computations; the fp64 reference's own error (about n_max * 2^-53) is far below what follows.
      sum_mag: a recursive fp32 sum of N non-negative terms in any order is within (N - 1) u relative
        of the exact sum (each of the N - 1 additions rounds once, no cancellation), to first order.
      offsets: the numerator sum(mag * o), |o| <= w, has terms rounded once (u each) and N - 1
        additions; its absolute error is within N u * w * S where S = sum mag bounds sum |mag * o| / w.
        Dividing by the computed S (relative error (N - 1) u) and rounding the quotient adds
        ((N - 1) u + u) * |result| <= N u w.  Together 2 N u w; the issue's figure is 2 (N - 1) u w
        "plus the division's rounding" -- the same to within u w.  A window of 0 gives exactly 0.
    A factor (1 + N u) for the second-order terms is below 5e-5 at N = 729 and is absorbed by taking
    N, not N - 1, throughout."""
    u = 2.0 ** -24
    n_max = max(int(n_max), 1)
    return n_max * u, tuple(2.0 * n_max * u * w for w in win)


def assert_mplots_match(got, want, win):
    """Count, order, frame, range, doppler, beam, n_merged and the bits of mag exact; sum_mag and the
    three offsets within tolerances() of this case's largest n_merged and its windows."""
    assert len(got) == len(want), (len(got), len(want))
    for name in ("frame", "range", "doppler", "beam", "n_merged"):
        np.testing.assert_array_equal(got[name], want[name], err_msg=name)
    np.testing.assert_array_equal(got["mag"].view(np.uint32), want["mag"].view(np.uint32), err_msg="mag")
    if not len(want):
        return
    rtol, atols = tolerances(want["n_merged"].max(), win)
    np.testing.assert_allclose(got["sum_mag"], want["sum_mag"], rtol=rtol, atol=0, err_msg="sum_mag")
    for name, atol in zip(("d_beam", "d_range", "d_doppler"), atols):
        np.testing.assert_allclose(got[name], want[name], rtol=0, atol=atol, err_msg=name)


# Hand-made lists on 3 beams of 8 x 8, small enough to check by eye: name -> (rows (frame m, range,
# doppler, mag), win, beam_wrap, the expected (scan, beam, range, doppler, n_merged) per merged plot).
HAND = {
    # one target seen in all three beams, strongest in the middle one
    "same_cell_three_beams": ([(0, 3, 3, 2.0), (1, 3, 3, 5.0), (2, 3, 3, 1.0)], (1, 1, 1), 0, [(0, 1, 3, 3, 3)]),
    # equal magnitudes: the earlier record wins, and it sees only the beam next to it
    "equal_mags": ([(0, 3, 3, 4.0), (1, 3, 3, 4.0), (2, 3, 3, 4.0)], (1, 1, 1), 0, [(0, 0, 3, 3, 2)]),
    # two targets sharing a cell in beams 0 and 2: on the circular axis of 3 beams they are neighbours
    # (one plot with win_beam 1, two with win_beam 0); clamped, beams 0 and 2 are two apart (two plots
    # with win_beam 1, one with win_beam 2)
    "share_cell_wrap_w1": ([(0, 3, 3, 5.0), (2, 3, 3, 4.0)], (1, 1, 1), 1, [(0, 0, 3, 3, 2)]),
    "share_cell_wrap_w0": ([(0, 3, 3, 5.0), (2, 3, 3, 4.0)], (0, 1, 1), 1, [(0, 0, 3, 3, 1), (0, 2, 3, 3, 1)]),
    "share_cell_clamp_w1": ([(0, 3, 3, 5.0), (2, 3, 3, 4.0)], (1, 1, 1), 0, [(0, 0, 3, 3, 1), (0, 2, 3, 3, 1)]),
    "share_cell_clamp_w2": ([(0, 3, 3, 5.0), (2, 3, 3, 4.0)], (2, 1, 1), 0, [(0, 0, 3, 3, 2)]),
    # the wrap turns within a scan: beam 2 of scan 0 (m = 2) and beam 0 of scan 1 (m = 3) never merge
    "wrap_stays_in_its_scan": ([(2, 3, 3, 5.0), (3, 3, 3, 4.0), (5, 3, 3, 3.0)], (1, 1, 1), 1,
                               [(0, 2, 3, 3, 1), (1, 0, 3, 3, 2)]),
    # Doppler columns 7 and 0 are neighbours, across beams too
    "doppler_wrap": ([(0, 3, 0, 2.0), (1, 3, 7, 5.0)], (1, 1, 1), 0, [(0, 1, 3, 7, 2)]),
    # range is clamped: rows 0 and 7 are not neighbours; rows 6 and 7 are
    "range_edge": ([(0, 0, 2, 1.0), (1, 7, 2, 3.0), (2, 6, 2, 2.0)], (1, 1, 1), 0, [(0, 0, 0, 2, 1), (0, 1, 7, 2, 2)]),
    # a chain A < B < C with C outside A's neighbourhood: only C is a peak
    "chain": ([(0, 3, 3, 1.0), (1, 3, 3, 2.0), (2, 3, 3, 3.0)], (1, 1, 1), 0, [(0, 2, 3, 3, 2)]),
    "chain_in_range": ([(0, 2, 3, 1.0), (1, 3, 3, 2.0), (2, 4, 3, 3.0), (4, 4, 4, 1.0)], (1, 1, 1), 0,
                       [(0, 2, 4, 3, 2), (1, 1, 4, 4, 1)]),
}


def hand_records(rows, dtype):
    """A record array of `dtype` (frame / range / doppler / mag fields) from HAND rows, sorted."""
    a = np.zeros(len(rows), dtype)
    for i, (m, r, d, mag) in enumerate(sorted(rows)):
        a["frame"][i], a["range"][i], a["doppler"][i], a["mag"][i] = m, r, d, mag
    return a


# ---- list generators of the host and the GPU tests ----
def random_list(seed, n_maps, nr, nd, density, dtype=DET_DTYPE, levels=5):
    rng = np.random.default_rng(seed)
    f, r, d = np.nonzero(rng.random((n_maps, nr, nd)) < density)
    a = np.zeros(len(f), dtype)
    a["frame"], a["range"], a["doppler"] = f, r, d
    a["mag"] = rng.integers(1, levels + 1, len(f)).astype(np.float32)
    return a


def tile_edge_list(n):
    """Exactly n records of 32 x 32 maps whose last record is in frame 3: merged as 2 scans x 3 beams,
    maps 4 and 5 are empty."""
    recs = thin_to(random_list(40, 4, 32, 32, 0.7), n, n)
    assert len(recs) == n and recs["frame"][-1] == 3, (len(recs), n, int(recs["frame"][-1]))
    return recs
