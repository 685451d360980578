"""The interference exciser's specification (include/fmcw.h "Interference excision") in NumPy float32:
every step one individually rounded fp32 operation, so the GPU result equals this bit for bit.  Also an
independent brute force (float64 sort for the level, a per-sample Python loop for the dilation, the runs
and the repair) that the host tests hold the restatement to.

Cubes are in RadarCore's conventions: complex64 [..., sample] for "f32", float16 / int16 [..., sample, 2]
for "f16" / "i16".  A line is the last sample axis; every leading axis is a batch of lines."""
import numpy as np

ZERO, INTERP = "zero", "interp"
F32 = np.float32


def dtype_of(cube) -> str:
    return {np.dtype(np.complex64): "f32", np.dtype(np.float16): "f16", np.dtype(np.int16): "i16"}[np.asarray(cube).dtype]


def components(cube):
    """(re, im) float32 [..., sample], converted exactly."""
    cube = np.asarray(cube)
    if cube.dtype == np.complex64:
        return np.ascontiguousarray(cube.real), np.ascontiguousarray(cube.imag)
    return cube[..., 0].astype(F32), cube[..., 1].astype(F32)


def from_components(re, im, like):
    """The fp32 components written back in the dtype of `like`: f16 to nearest even, int16 half to even."""
    if like.dtype == np.complex64:
        out = np.empty(re.shape, np.complex64)
        out.real, out.imag = re, im
        return out
    if like.dtype == np.int16:
        re, im = np.rint(re), np.rint(im)
    return np.stack([re, im], axis=-1).astype(like.dtype)


def power(cube):
    re, im = components(cube)
    return re * re + im * im          # float32 arrays: each product and the sum rounded once


def rank_of(ns: int, rank_pct: int) -> int:
    return ns * rank_pct // 100


def level(p, rank_pct=50):
    k = rank_of(p.shape[-1], rank_pct)
    return np.partition(p, k, axis=-1)[..., k]


def flags(p, rank_pct=50, alpha=16.0):
    t = F32(alpha) * level(p, rank_pct)
    return p > t[..., None]


def dilate(f, guard=4):
    g = f.copy()
    for s in range(1, guard + 1):
        g[..., s:] |= f[..., :-s]
        g[..., :-s] |= f[..., s:]
    return g


def runs_of(g_line):
    """[(a, b)] of the maximal runs of a bool line, inclusive."""
    d = np.diff(np.concatenate([[0], g_line.astype(np.int8), [0]]))
    return list(zip(np.flatnonzero(d == 1).tolist(), (np.flatnonzero(d == -1) - 1).tolist()))


def mask_words(g):
    """uint32 [..., Ns / 32]: bit n % 32 of word n / 32 = g[n]."""
    return np.packbits(g, axis=-1, bitorder="little").view("<u4")


def excise(cube, mode=ZERO, guard=4, rank_pct=50, alpha=16.0):
    """(repaired cube, g bool [..., sample], counts uint32 [...], status uint32[4])."""
    cube = np.ascontiguousarray(cube)
    p = power(cube)
    ns = p.shape[-1]
    f = flags(p, rank_pct, alpha)
    g = dilate(f, guard)
    re, im = components(cube)
    re, im = re.reshape(-1, ns).copy(), im.reshape(-1, ns).copy()
    g2 = g.reshape(-1, ns)
    for i in np.flatnonzero(g2.any(axis=-1)):
        for a, b in runs_of(g2[i]):
            for x in (re[i], im[i]):
                has_lo, has_hi = a > 0, b < ns - 1
                if mode == ZERO or not (has_lo or has_hi):
                    x[a:b + 1] = 0
                elif not has_hi:
                    x[a:b + 1] = x[a - 1]
                elif not has_lo:
                    x[a:b + 1] = x[b + 1]
                else:
                    lo, hi = x[a - 1], x[b + 1]
                    t = np.arange(1, b - a + 2).astype(F32) / F32(b - a + 2)
                    d = hi - lo
                    x[a:b + 1] = lo + t * d
    fixed = from_components(re, im, cube).reshape(cube.shape)
    out = cube.copy()
    sel = g if cube.dtype == np.complex64 else g[..., None] & np.ones(2, bool)
    out[sel] = fixed[sel]               # samples outside every run keep their bits
    counts = g.sum(axis=-1).astype(np.uint32)
    status = np.array([counts.sum(), (counts > 0).sum(), f.sum(), (counts > ns // 2).sum()], np.uint32)
    return out, g, counts, status


def brute_force(cube, mode=ZERO, guard=4, rank_pct=50, alpha=16.0):
    """The same outputs for one line [sample] (or [sample, 2]), by the definitions: the level from a
    float64 sort, the dilation, the runs and the repair sample by sample."""
    cube = np.asarray(cube)
    re, im = components(cube)
    ns = len(re)
    p = [F32(F32(re[n] * re[n]) + F32(im[n] * im[n])) for n in range(ns)]
    m = F32(sorted(float(v) for v in p)[ns * rank_pct // 100])
    t = F32(F32(alpha) * m)
    f = [bool(v > t) for v in p]
    g = [any(f[j] for j in range(max(0, n - guard), min(ns, n + guard + 1))) for n in range(ns)]
    ore, oim = re.copy(), im.copy()
    for n in range(ns):
        if not g[n]:
            continue
        a = n
        while a > 0 and g[a - 1]:
            a -= 1
        b = n
        while b < ns - 1 and g[b + 1]:
            b += 1
        for src, dst in ((re, ore), (im, oim)):
            if mode == ZERO or (a == 0 and b == ns - 1):
                dst[n] = 0
            elif b == ns - 1:
                dst[n] = src[a - 1]
            elif a == 0:
                dst[n] = src[b + 1]
            else:
                lo, hi = F32(src[a - 1]), F32(src[b + 1])
                tt = F32(F32(n - a + 1) / F32(b - a + 2))
                dst[n] = F32(lo + F32(tt * F32(hi - lo)))
    fixed = from_components(ore, oim, cube)
    out = cube.copy()
    for n in range(ns):
        if g[n]:
            out[n] = fixed[n]
    g = np.array(g)
    return out, g, np.uint32(g.sum()), np.array([g.sum(), g.any(), sum(f), g.sum() > ns // 2], np.uint32)
