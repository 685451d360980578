"""The clutter map of include/fmcw.h ("Clutter map") restated in NumPy float32: the specification of
tests/test_cmap_host.py and tests/test_gpu_cmap.py, never derived from the code under test.  Every array
operation below is one IEEE fp32 operation per element (NumPy has no fused multiply-add), so the result
is the header's bit for bit.
"""
import numpy as np

DET_DTYPE = np.dtype([("frame", "<u4"), ("range", "<u2"), ("doppler", "<u2"), ("mag", "<f4"), ("threshold", "<f4")])
AGE_MAX = 0xFFFFFFFF
DEFAULTS = dict(n_streams=1, gain=0.125, alpha=4.0, floor=0.0, clip=0.0, spread=(1, 1), warmup=8)


def nonneg(m):
    """Negative cells and -0.0 become +0 (the integer maximum on the bit pattern, as det_sink.hpp)."""
    m = np.ascontiguousarray(m, dtype=np.float32)
    return np.maximum(m.view(np.int32), 0).view(np.float32)


def neighbourhood_max(c, spread):
    """M[r][d] = max of c[r+dr][(d+dd) mod nd], |dr| <= Sr with 0 <= r+dr < nr, |dd| <= Sd."""
    sr, sd = spread
    nr = c.shape[0]
    h = c.copy()
    for dd in range(1, sd + 1):
        h = np.maximum(h, np.maximum(np.roll(c, dd, axis=1), np.roll(c, -dd, axis=1)))
    m = h.copy()
    for dr in range(1, sr + 1):
        m[dr:] = np.maximum(m[dr:], h[:nr - dr])      # row r - dr
        m[:nr - dr] = np.maximum(m[:nr - dr], h[dr:])  # row r + dr
    return m


def scan(c, a, m, gain=0.125, alpha=4.0, floor=0.0, clip=0.0, spread=(1, 1), warmup=8):
    """One scan of one stream: (hit mask or None, x, T or None, c', a')."""
    f32 = np.float32
    x = nonneg(m)
    if a == 0:
        return None, x, None, x.copy(), 1
    big = neighbourhood_max(c, spread)
    t = np.maximum(f32(alpha) * big, f32(floor))
    hit = (x > t) if a >= warmup else None
    u = x if clip == 0 else np.minimum(x, np.maximum(f32(clip) * c, f32(floor)))
    d = u - c
    p = f32(gain) * d
    cn = c + p
    assert t.dtype == d.dtype == p.dtype == cn.dtype == np.float32
    return hit, x, t, cn, min(a + 1, AGE_MAX)


def detect(maps, n_streams=1, gain=0.125, alpha=4.0, floor=0.0, clip=0.0, spread=(1, 1), warmup=8, state=None):
    """maps: float32 [frame][range][doppler], frame f belonging to stream f % n_streams; state: (planes
    [stream][range][doppler], ages [stream]) or None for a fresh map.  Returns (the ordered DET_DTYPE
    list, planes, ages); the state given is left unchanged."""
    maps = np.asarray(maps, np.float32)
    if maps.ndim == 2:
        maps = maps[None]
    nf, nr, nd = maps.shape
    assert nf % n_streams == 0
    if state is None:
        planes, ages = np.zeros((n_streams, nr, nd), np.float32), np.zeros(n_streams, np.uint32)
    else:
        planes, ages = np.array(state[0], np.float32), np.array(state[1], np.uint32)
    ages = [int(a) for a in ages]
    out = []
    for f in range(nf):
        b = f % n_streams
        hit, x, t, planes[b], ages[b] = scan(planes[b], ages[b], maps[f], gain, alpha, floor, clip, spread, warmup)
        if hit is None:
            continue
        r, d = np.nonzero(hit)                 # row-major: (range, doppler) ascending
        rec = np.zeros(len(r), DET_DTYPE)
        rec["frame"], rec["range"], rec["doppler"] = f, r, d
        rec["mag"], rec["threshold"] = x[hit], t[hit]
        out.append(rec)
    dets = np.concatenate(out) if out else np.zeros(0, DET_DTYPE)
    return dets, planes, np.array(ages, np.uint32)
