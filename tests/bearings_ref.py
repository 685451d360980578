"""The bearing estimator's specification (include/fmcw.h, "Bearing estimation") in fp64 NumPy, and
the derived tolerances the GPU tests hold fmcw_bearings_enqueue to.

    s_k   = sum_c w[c] y_k[c] exp(-2 pi i d c / n_doppler)         y_k: MTI canceller over spec[f][k][r][:]
    P     = sum_k s_{k+1} conj(s_k);  nu = arg(P) / 2 pi;  sin_theta = nu / spacing
    power = sqrt(sum_k |s_k|^2);      coherence = |P| / sum_k |s_{k+1}| |s_k|

Tolerances (assert_bearings_match), eps = 2^-24:
    s_k        |s_gpu - s_ref| <= e_k = 40 eps A_k,  A_k = sum_c w[c] (|x[c]| + m1 |x[c-1]| + m2 |x[c-2]|),
               (m1, m2) the canceller's coefficients: about 5 roundings per term, up to 16 sequential
               adds per lane and 6 tree adds, with slack
    power      the 2-norm of the e_k
    nu         asin(min(1, E_P / |P|)) / 2 pi + 2^-20 cycles (circular difference),
               E_P = sum_k |s_{k+1}| e_k + |s_k| e_{k+1} + e_k e_{k+1}; a record with E_P / |P| > 0.05
               is ill-conditioned and skipped for nu only, at most 5 % of a list
    coherence  2 E_P / |P|  (numerator and denominator each move by at most E_P, and the denominator
               is at least |P|)
    frame, range, doppler, flags: exact.
"""
import numpy as np

EPS = 2.0 ** -24
FLAG_NO_ANGLE, FLAG_ONE_RX, FLAG_OUT_OF_RANGE = 1, 2, 4
MTI_COEF = {0: (0.0, 0.0), 2: (1.0, 0.0), 3: (2.0, 1.0)}

REF_DTYPE = np.dtype([("frame", "<u4"), ("range", "<u2"), ("doppler", "<u2"), ("flags", "<u4"),
                      ("nu", "<f8"), ("sin_theta", "<f8"), ("power", "<f8"), ("coherence", "<f8")])


def window(n: int, kind: str = "hamming") -> np.ndarray:
    """The library's fp32 Doppler window as fp64 values: Hamming 0.54 - 0.46 cos(2 pi a / (n - 1)) on the
    mirrored half address, rounded to fp32; ones for "none"."""
    if kind == "none":
        return np.ones(n)
    i = np.arange(n)
    a = np.minimum(np.where(i < n // 2, i, n - 1 - i), n // 2 - 1)
    return (0.54 - 0.46 * np.cos(2.0 * np.pi * a / (n - 1))).astype(np.float32).astype(np.float64)


def _delayed(x, k):
    y = np.zeros_like(x)
    y[..., k:] = x[..., :-k]
    return y


def snapshots(spec, f, r, d, win="hamming", mti=0):
    """s [n, n_rx] complex128 and the bound sums A [n, n_rx] for cells (f, r, d) (all in range) of
    spec [frame][rx][range][chirp]."""
    spec = np.asarray(spec)
    nc = spec.shape[-1]
    x = spec[np.asarray(f, np.int64), :, np.asarray(r, np.int64), :].astype(np.complex128)   # [n, rx, chirp]
    m1, m2 = MTI_COEF[mti]
    x1, x2 = _delayed(x, 1), _delayed(x, 2)
    y = x - m1 * x1 + m2 * x2
    w = window(nc, win)
    m = (np.asarray(d, np.int64)[:, None] * np.arange(nc)[None, :]) % nc
    tw = np.exp(-2j * np.pi * m / nc)[:, None, :]
    s = (w * y * tw).sum(axis=-1)
    a = (w * (np.abs(x) + m1 * np.abs(x1) + m2 * np.abs(x2))).sum(axis=-1)
    return s, a


def from_snapshots(s, spacing=0.5):
    """(nu, sin_theta, power, coherence, P, flags) in fp64 from snapshots [n, n_rx]."""
    s = np.asarray(s, np.complex128)
    n, nrx = s.shape
    power = np.sqrt((np.abs(s) ** 2).sum(axis=1))
    flags = np.zeros(n, np.uint32)
    if nrx == 1:
        z = np.zeros(n)
        return z, z.copy(), power, z.copy(), np.zeros(n, np.complex128), flags | FLAG_ONE_RX
    p = (s[:, 1:] * np.conj(s[:, :-1])).sum(axis=1)
    den = (np.abs(s[:, 1:]) * np.abs(s[:, :-1])).sum(axis=1)
    nu = np.angle(p) / (2.0 * np.pi)
    ok = (den > 0) & np.isfinite(den)
    coh = np.where(ok, np.abs(p) / np.where(ok, den, 1.0), 0.0)
    st = nu / spacing
    flags[np.abs(st) > 1.0] |= FLAG_NO_ANGLE
    return nu, st, power, coh, p, flags


def bearings_ref(spec, records, n_frames=None, win="hamming", mti=0, spacing=0.5):
    """The specification on a record list (any structured array with frame / range / doppler):
    (REF_DTYPE array, snapshots [n, n_rx] complex128, bound sums A [n, n_rx]).  Out-of-range records
    (frame >= n_frames, default all of spec) read nothing: zeros and flag 4."""
    spec = np.asarray(spec)
    nf, nrx, nr, nc = spec.shape
    nf = nf if n_frames is None else n_frames
    f, r, d = (np.asarray(records[k], np.int64) for k in ("frame", "range", "doppler"))
    n = len(f)
    good = (f < nf) & (r < nr) & (d < nc)
    out = np.zeros(n, REF_DTYPE)
    s = np.zeros((n, nrx), np.complex128)
    a = np.zeros((n, nrx))
    out["flags"][~good] = FLAG_OUT_OF_RANGE
    if good.any():
        s[good], a[good] = snapshots(spec, f[good], r[good], d[good], win, mti)
        nu, st, pw, coh, _, fl = from_snapshots(s[good], spacing)
        for k, v in (("frame", f[good]), ("range", r[good]), ("doppler", d[good]), ("flags", fl), ("nu", nu),
                     ("sin_theta", st), ("power", pw), ("coherence", coh)):
            out[k][good] = v
    return out, s, a


def assert_bearings_match(got, got_snaps, ref, ref_s, ref_a, spacing=0.5, label=""):
    """got (BEARING_DTYPE) and got_snaps (complex64 [n, n_rx], or None) against bearings_ref's triple,
    within the module docstring's bounds.  Returns the worst fraction of each bound used:
    {"s", "power", "nu", "coherence", "cond" (worst E_P / |P|), "skipped"}."""
    n, nrx = ref_s.shape
    assert len(got) == n, (len(got), n)
    for k in ("frame", "range", "doppler", "flags"):
        np.testing.assert_array_equal(got[k], ref[k], err_msg=f"{label} {k}")
    assert not np.any(got["reserved"])
    used = {"s": 0.0, "power": 0.0, "nu": 0.0, "coherence": 0.0, "cond": 0.0, "skipped": 0}
    good = (ref["flags"] & FLAG_OUT_OF_RANGE) == 0
    bad = ~good
    for k in ("nu", "sin_theta", "power", "coherence"):
        assert not np.any(got[k][bad]), f"{label} {k} of an out-of-range record"
    if got_snaps is not None:
        assert got_snaps.shape == (n, nrx)
        assert not np.any(got_snaps[bad])
    if not good.any():
        return used
    e = 40.0 * EPS * ref_a[good]
    s = ref_s[good]
    g = got[good]
    tiny = np.finfo(np.float64).tiny
    if got_snaps is not None:
        frac = np.abs(got_snaps[good].astype(np.complex128) - s) / np.maximum(e, tiny)
        used["s"] = float(frac.max())
        assert used["s"] <= 1.0, f"{label} snapshot error {used['s']:.3f} of its bound"
    frac = np.abs(g["power"].astype(np.float64) - ref["power"][good]) / np.maximum(np.sqrt((e ** 2).sum(axis=1)), tiny)
    used["power"] = float(frac.max())
    assert used["power"] <= 1.0, f"{label} power error {used['power']:.3f} of its bound"
    if nrx == 1:
        assert not np.any(g["nu"]) and not np.any(g["sin_theta"]) and not np.any(g["coherence"])
        return used
    a = np.abs(s)
    e_p = (a[:, 1:] * e[:, :-1] + a[:, :-1] * e[:, 1:] + e[:, :-1] * e[:, 1:]).sum(axis=1)
    p = (s[:, 1:] * np.conj(s[:, :-1])).sum(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        cond = np.where(np.abs(p) > 0, e_p / np.abs(p), np.inf)
    well = cond <= 0.05
    used["skipped"] = int((~well).sum())
    assert used["skipped"] <= 0.05 * len(cond), f"{label} {used['skipped']} of {len(cond)} records ill-conditioned"
    if well.any():
        used["cond"] = float(cond[well].max())
        tol = np.arcsin(np.minimum(1.0, cond[well])) / (2.0 * np.pi) + 2.0 ** -20
        diff = (g["nu"][well].astype(np.float64) - ref["nu"][good][well] + 0.5) % 1.0 - 0.5
        used["nu"] = float((np.abs(diff) / tol).max())
        assert used["nu"] <= 1.0, f"{label} nu error {used['nu']:.3f} of its bound"
        # sin_theta is nu / spacing in fp32: one more rounding of a value below 1 / spacing
        st = g["nu"][well].astype(np.float64) / spacing
        assert np.all(np.abs(g["sin_theta"][well] - st) <= 4 * EPS * np.maximum(np.abs(st), 1.0)), f"{label} sin_theta"
    assert np.all(np.abs(g["nu"]) <= 0.5)
    fin = np.isfinite(cond)
    if fin.any():
        frac = np.abs(g["coherence"][fin].astype(np.float64) - ref["coherence"][good][fin]) / (2.0 * cond[fin])
        used["coherence"] = float(frac.max())
        assert used["coherence"] <= 1.0, f"{label} coherence error {used['coherence']:.3f} of its bound"
    return used


# ---- the full-scale cases (tests/test_gpu_bearings.py), checked on the CPU by tests/test_bearings_host.py ----
FS_NF, FS_NR, FS_NRX = 2, 64, 4
FS_DOPPLERS = [32, 1024]                  # half the wave idle in a 64-chirp step; 16 steps a row
FS_MTIS = [0, 2, 3]
FS_BINS = 8                               # records per (frame, range row)


def full_scale_records(n_frames, n_range, n_doppler):
    """A record list (frame / range / doppler) that is no detection list: FS_BINS cells in every range
    row of every frame, n_doppler / FS_BINS apart, the first one moving on by one bin from row to row
    and on through the frames, so that the list visits every Doppler bin as well."""
    step = n_doppler // FS_BINS
    assert n_frames * n_range >= step
    f, r, j = np.meshgrid(np.arange(n_frames), np.arange(n_range), np.arange(FS_BINS), indexing="ij")
    recs = np.zeros(f.size, np.dtype([("frame", "<u4"), ("range", "<u2"), ("doppler", "<u2"),     # fmcw.DET_DTYPE
                                      ("mag", "<f4"), ("threshold", "<f4")]))
    recs["frame"], recs["range"] = f.ravel(), r.ravel()
    recs["doppler"] = (j * step + (r + n_range * f) % step).ravel()
    return recs


def full_scale_case(nc, mti):
    """(spec, recs, win): beams_ref.full_scale_spec with the list above; the window alternates."""
    from beams_ref import full_scale_spec
    win = ("hamming", "none")[(FS_DOPPLERS.index(nc) + FS_MTIS.index(mti)) % 2]
    return full_scale_spec(FS_NF, FS_NRX, FS_NR, nc, seed=8000 + nc), full_scale_records(FS_NF, FS_NR, nc), win
