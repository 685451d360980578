"""NumPy restatement of the plot extractor's specification (include/fmcw.h, fmcw_plots_*), with
fp64 sums.  A helper for test_plots_host.py / test_gpu_plots.py, not a test module.

Input: a DET_DTYPE array strictly increasing in (frame, range, doppler).  The window of
P = (f, r, d) is every detection (f, r + dr, (d + dd) mod n_doppler) with |dr| <= win_range,
|dd| <= win_doppler, 0 <= r + dr < n_range (Doppler circular, range clamped, P included).  P is a
peak iff for every other Q of its window mag(P) > mag(Q), or mag(P) == mag(Q) and P precedes Q in
the list.  One plot per peak, in list order.
"""
import numpy as np

PLOT_REF_DTYPE = np.dtype([("frame", "<u4"), ("range", "<u2"), ("doppler", "<u2"), ("mag", "<f4"),
                           ("threshold", "<f4"), ("n_cells", "<u4"), ("sum_mag", "<f8"),
                           ("d_range", "<f8"), ("d_doppler", "<f8")])


def plots_ref(dets, n_range, n_doppler, win_range, win_doppler):
    assert n_doppler >= 2 * win_doppler + 1
    n = len(dets)
    fr = dets["frame"].astype(np.int64)
    rg = dets["range"].astype(np.int64)
    dp = dets["doppler"].astype(np.int64)
    mag = dets["mag"]
    key = (fr * n_range + rg) * n_doppler + dp
    assert np.all(np.diff(key) > 0), "list must be strictly increasing in (frame, range, doppler)"
    idx = np.arange(n)
    peak = np.ones(n, bool)
    cells = np.zeros(n, np.int64)
    s = np.zeros(n, np.float64)
    sr = np.zeros(n, np.float64)
    sd = np.zeros(n, np.float64)
    for dr in range(-win_range, win_range + 1):
        ok_row = (rg + dr >= 0) & (rg + dr < n_range)
        for dd in range(-win_doppler, win_doppler + 1):
            qkey = (fr * n_range + rg + dr) * n_doppler + (dp + dd) % n_doppler
            q = np.searchsorted(key, qkey)
            hit = ok_row & (q < n)
            hit[hit] = key[q[hit]] == qkey[hit]
            p, q = idx[hit], q[hit]
            mq = mag[q]
            cells[p] += 1
            s[p] += mq.astype(np.float64)
            sr[p] += mq.astype(np.float64) * dr
            sd[p] += mq.astype(np.float64) * dd
            other = q != p
            beaten = other & ((mq > mag[p]) | ((mq == mag[p]) & (q < p)))
            peak[p[beaten]] = False
    out = np.zeros(int(peak.sum()), PLOT_REF_DTYPE)
    k = idx[peak]
    for name in ("frame", "range", "doppler", "mag", "threshold"):
        out[name] = dets[name][k]
    out["n_cells"] = cells[k]
    out["sum_mag"] = s[k]
    good = np.isfinite(s[k]) & (s[k] != 0)
    den = np.where(good, s[k], 1.0)
    out["d_range"] = np.where(good, sr[k] / den, 0.0)
    out["d_doppler"] = np.where(good, sd[k] / den, 0.0)
    return out


def assert_plots_match(got, want):
    """The issue's tolerances: identity fields, mag / threshold bits, n_cells, order and count
    exact; sum_mag within 1e-5 relative (<= 81 positive fp32 terms: 80 * 2^-24 in any order);
    d_range / d_doppler within 1e-4 bins (81 * 2^-24 * 4 for the numerator + 4 * 4.8e-6)."""
    assert len(got) == len(want), (len(got), len(want))
    for name in ("frame", "range", "doppler", "n_cells"):
        np.testing.assert_array_equal(got[name], want[name], err_msg=name)
    for name in ("mag", "threshold"):
        np.testing.assert_array_equal(got[name].view(np.uint32), want[name].view(np.uint32), err_msg=name)
    np.testing.assert_allclose(got["sum_mag"], want["sum_mag"], rtol=1e-5, atol=0)
    np.testing.assert_allclose(got["d_range"], want["d_range"], rtol=0, atol=1e-4)
    np.testing.assert_allclose(got["d_doppler"], want["d_doppler"], rtol=0, atol=1e-4)
