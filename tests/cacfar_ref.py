"""The cell-averaging CFAR of include/fmcw.h ("Cell-averaging CFAR") restated in NumPy float32: the
specification of tests/test_cacfar_host.py and tests/test_gpu_cacfar.py, never derived from the code
under test.  Every array operation below is one IEEE fp32 operation per element, in the header's
canonical order, so the result is the header's bit for bit.
"""
import numpy as np

DET_DTYPE = np.dtype([("frame", "<u4"), ("range", "<u2"), ("doppler", "<u2"), ("mag", "<f4"), ("threshold", "<f4")])
MODES = ("ca", "go", "so")


def n_ref(ref, guard):
    (rr, rd), (gr, gd) = ref, guard
    return (2 * (rr + gr) + 1) * (2 * (rd + gd) + 1) - (2 * gr + 1) * (2 * gd + 1)


def nonneg(m):
    """Negative cells and -0.0 become +0 (the integer maximum on the bit pattern, as det_sink.hpp)."""
    m = np.ascontiguousarray(m, dtype=np.float32)
    return np.maximum(m.view(np.int32), 0).view(np.float32)


def _sum(x, axis, lo, hi):
    """sum of x[.. i + k ..] for k = lo .. hi in ascending order along `axis` (circular); +0 if empty."""
    s = None
    for k in range(lo, hi + 1):
        t = np.roll(x, -k, axis=axis)
        s = t if s is None else s + t
    return np.zeros_like(x) if s is None else s


def thresholds(maps, mode="ca", ref=(4, 4), guard=(1, 2), alpha=4.0):
    """(clamped maps, T, tested) for float32 maps [..][range][doppler].  T is meaningful in the tested
    rows only (the range shifts wrap around elsewhere)."""
    (rr, rd), (gr, gd) = ref, guard
    hr, hd = rr + gr, rd + gd
    n = n_ref(ref, guard)
    m = nonneg(maps)
    nr, nd = m.shape[-2:]
    assert n >= 2 and 2 * hd + 1 <= nd and 2 * hr + 1 <= nr
    lg = _sum(m, -1, -hd, -gd - 1)
    cg = _sum(m, -1, -gd, gd)
    rg = _sum(m, -1, gd + 1, hd)
    h = (lg + cg) + rg
    u = _sum(h, -2, -hr, -gr - 1)
    d = _sum(h, -2, gr + 1, hr)
    l = _sum(lg, -2, -gr, gr)
    r = _sum(rg, -2, -gr, gr)
    a, b = u + l, d + r
    with np.errstate(invalid="ignore", over="ignore"):
        if mode == "ca":
            t = np.float32(np.float64(np.float32(alpha)) / n) * (a + b)
        else:
            kh = np.float32(np.float64(np.float32(alpha)) / (n // 2))
            t = kh * (np.maximum(a, b) if mode == "go" else np.minimum(a, b))
    assert t.dtype == np.float32
    tested = np.zeros(m.shape, bool)
    tested[..., hr:nr - hr, :] = True
    return m, t, tested


def detect(maps, mode="ca", ref=(4, 4), guard=(1, 2), alpha=4.0):
    """The ordered DET_DTYPE list of float32 maps [frame][range][doppler] (or one map)."""
    maps = np.asarray(maps, np.float32)
    if maps.ndim == 2:
        maps = maps[None]
    m, t, tested = thresholds(maps, mode, ref, guard, alpha)
    with np.errstate(invalid="ignore"):
        hit = tested & (m > t)
    f, r, d = np.nonzero(hit)              # row-major: (frame, range, doppler) ascending
    out = np.zeros(len(f), DET_DTYPE)
    out["frame"], out["range"], out["doppler"] = f, r, d
    out["mag"], out["threshold"] = m[hit], t[hit]
    return out
