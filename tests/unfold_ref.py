"""NumPy / plain-integer restatement of the velocity unfolder's specification (include/fmcw.h,
fmcw_unfold_*): integers only (Python's, unbounded) except the one fp32 sum.  A helper for
test_unfold_host.py / test_gpu_unfold.py, not a test module.

A dwell is K consecutive scans of one stream, one per PRF of the stagger.  PRF k is p_k f0; the fine
unit of frequency is f0 / Nc, so one Doppler bin of PRF k is p_k fine units and a record at bin d of
PRF k stands for the velocities v_m = (ds + m Nc) p_k, ds the signed bin.  A hypothesis is a hit at
another position of the dwell when that scan holds a record where v_m folds to at that scan's PRF
(within the tolerances).  The hypothesis with the most hits wins, and the earliest scan that sees
the target owns the report.

Output order: (dwell, stream, then list order of P within that stream's scans of the dwell), so that
the output's .frame = j n_streams + t never decreases, which is what the device tracker asks of its
input.  With one stream this is "dwell, then list order".
"""
from dataclasses import dataclass

import numpy as np

import scenario_ref as S
from fmcw import DET_DTYPE, synth
from tile_edge import thin_to

VPLOT_REF_DTYPE = np.dtype([("frame", "<u4"), ("range", "<u2"), ("doppler", "<u2"), ("mag", "<f4"),
                            ("v_fine", "<i4"), ("fold", "<i2"), ("n_hits", "u1"), ("hit_mask", "u1"),
                            ("sum_mag", "<f4"), ("pos", "<u2"), ("n_ties", "<u2"), ("src", "<u4")])
assert VPLOT_REF_DTYPE.itemsize == 32


@dataclass(frozen=True)
class Cfg:
    n_range: int = 1024
    n_doppler: int = 128
    prf_units: tuple = (8, 9, 10)          # K = len(prf_units)
    prf_phase: int = 0
    step: int = 3
    zero_bin: int = 0
    v_max: int = 2 * 128 * 8
    out_unit: int = 8
    tol_range: int = 1
    tol_doppler: int = 1
    m_of: int = 2
    n_streams: int = 1

    @property
    def n_prf(self):
        return len(self.prf_units)

    def check(self):
        K, nc = self.n_prf, self.n_doppler
        assert 1 <= self.n_range <= 65536 and 2 * self.tol_doppler + 1 <= nc <= 65536
        assert 2 <= K <= 8 and all(1 <= p <= 4096 for p in self.prf_units) and len(set(self.prf_units)) == K
        assert 0 <= self.prf_phase < K and 1 <= self.step <= K and 0 <= self.zero_bin < nc
        assert 0 <= self.v_max <= 32 * nc * min(self.prf_units)
        assert 1 <= self.out_unit <= 65535 and 2 * self.v_max // self.out_unit + 1 <= 65535
        assert 0 <= self.tol_range <= 4 and 0 <= self.tol_doppler <= 4 and 1 <= self.m_of <= K
        assert 1 <= self.n_streams <= 4096


def n_dwells(n_scans, K, step):
    return (n_scans - K) // step + 1 if n_scans >= K else 0


def signed_bin(d, zero_bin, nc):
    ds = (d - zero_bin) % nc
    return ds - nc if ds >= (nc + 1) // 2 else ds


def hypotheses(ds, nc, p, v_max):
    """[(m, v_m)] with |v_m| <= v_max, ascending m."""
    lim = v_max // p                       # |ds + m nc| <= lim
    m_lo = -((lim + ds) // nc)             # ceil((-lim - ds) / nc)
    m_hi = (lim - ds) // nc
    return [(m, (ds + m * nc) * p) for m in range(m_lo, m_hi + 1)]


def predicted_bin(v, p, zero_bin, nc):
    return ((2 * v + p) // (2 * p) + zero_bin) % nc


def out_doppler(v, v_max, u):
    return (2 * (v + v_max) + u) // (2 * u)


def unfold_ref(recs, n_scans, cfg: Cfg):
    """(vplots, status words 2 and 3: records at or beyond frame n_scans * n_streams, reports with
    n_ties > 1).  recs: any dtype with frame / range / doppler / mag, strictly increasing in (frame,
    range, doppler)."""
    cfg.check()
    K, nc, ns = cfg.n_prf, cfg.n_doppler, cfg.n_streams
    frames = [int(x) for x in recs["frame"]]
    n = 0
    while n < len(frames) and frames[n] < n_scans * ns:
        n += 1
    assert all(f >= n_scans * ns for f in frames[n:])
    beyond = len(frames) - n
    rg = [int(x) for x in recs["range"][:n]]
    dp = [int(x) for x in recs["doppler"][:n]]
    mag = np.asarray(recs["mag"][:n], np.float32)
    keys = [(frames[i], rg[i], dp[i]) for i in range(n)]
    assert all(a < b for a, b in zip(keys, keys[1:])), "list must be strictly increasing in (frame, range, doppler)"
    cell = {k: i for i, k in enumerate(keys)}
    by_frame = {}
    for i in range(n):
        by_frame.setdefault(frames[i], []).append(i)

    def window_hit(frame, r, d):
        """Index of the largest record of the window round (r, d) in `frame`, the first in list order
        among equals; None if the window is empty."""
        best = None
        for dr in range(-cfg.tol_range, cfg.tol_range + 1):
            rr = r + dr
            if not 0 <= rr < cfg.n_range:
                continue
            for dd in range(-cfg.tol_doppler, cfg.tol_doppler + 1):
                q = cell.get((frame, rr, (d + dd) % nc))
                if q is None:
                    continue
                if best is None or mag[q] > mag[best] or (mag[q] == mag[best] and q < best):
                    best = q
        return best

    out, tied = [], 0
    for j in range(n_dwells(n_scans, K, cfg.step)):
        for t in range(ns):
            for i in range(K):
                s = j * cfg.step + i
                p = cfg.prf_units[(s + cfg.prf_phase) % K]
                for P in by_frame.get(s * ns + t, []):
                    ds = signed_bin(dp[P], cfg.zero_bin, nc)
                    best = None        # (n_hits, v, m, mask, hit records by position)
                    ties = 0
                    for m, v in hypotheses(ds, nc, p, cfg.v_max):
                        hits = {i: P}
                        for i2 in range(K):
                            if i2 == i:
                                continue
                            s2 = j * cfg.step + i2
                            p2 = cfg.prf_units[(s2 + cfg.prf_phase) % K]
                            q = window_hit(s2 * ns + t, rg[P], predicted_bin(v, p2, cfg.zero_bin, nc))
                            if q is not None:
                                hits[i2] = q
                        nh = len(hits)
                        if best is None or nh > best[0]:
                            ties = 1
                        elif nh == best[0]:
                            ties += 1
                        if best is None or nh > best[0] or (nh == best[0] and abs(v) < abs(best[1])):
                            best = (nh, v, m, sum(1 << k for k in hits), hits)
                    if best is None or best[0] < cfg.m_of or min(best[4]) < i:
                        continue
                    nh, v, m, mask, hits = best
                    sm = np.float32(0)
                    for k in sorted(hits):
                        sm = np.float32(sm + mag[hits[k]])
                    ties = min(ties, 65535)
                    tied += int(ties > 1)
                    out.append((j * ns + t, rg[P], out_doppler(v, cfg.v_max, cfg.out_unit), mag[P], v, m, nh, mask,
                                sm, i, ties, P))
    return np.array(out, VPLOT_REF_DTYPE), beyond, tied


def assert_vplots_equal(got, want):
    """Record for record, every field; mag and sum_mag bit for bit."""
    assert len(got) == len(want), (len(got), len(want))
    for name in VPLOT_REF_DTYPE.names:
        a, b = got[name], want[name]
        if name in ("mag", "sum_mag"):
            a, b = a.view(np.uint32), b.view(np.uint32)
        np.testing.assert_array_equal(a, b, err_msg=name)


def records(rows, dtype):
    """A record array of `dtype` (frame / range / doppler / mag fields) from (frame, range, doppler,
    mag) rows, sorted."""
    a = np.zeros(len(rows), dtype)
    for i, (m, r, d, mag) in enumerate(sorted(rows)):
        a["frame"][i], a["range"][i], a["doppler"][i], a["mag"][i] = m, r, d, mag
    return a


def random_list(seed, n_frames, nr, nd, n_recs, dtype, levels=5, targets=6, cfg: Cfg = None, frame0=0):
    """About n_recs records over n_frames frames: uniform clutter with magnitudes from {1..levels}
    (ties everywhere), plus, when cfg is given, `targets` movers per stream written at the bins
    their velocity folds to in each scan (magnitude levels + 1 .. levels + 3), so that hypotheses with
    K hits exist."""
    rng = np.random.default_rng(seed)
    grid = np.zeros((n_frames, nr, nd), np.float32)
    pick = rng.random(grid.shape) < n_recs / grid.size
    grid[pick] = rng.integers(1, levels + 1, int(pick.sum()))
    if cfg is not None:
        K, ns = cfg.n_prf, cfg.n_streams
        for t in range(ns):
            for _ in range(targets):
                r = int(rng.integers(0, nr))
                v = int(rng.integers(-cfg.v_max, cfg.v_max + 1)) if cfg.v_max else 0
                for s in range(n_frames // ns):
                    if rng.random() < 0.2:
                        continue                      # a missed scan
                    p = cfg.prf_units[(s + cfg.prf_phase) % K]
                    grid[s * ns + t, r, predicted_bin(v, p, cfg.zero_bin, nd)] = levels + 1 + int(rng.integers(0, 3))
    f, r, d = np.nonzero(grid)
    a = np.zeros(len(f), dtype)
    a["frame"], a["range"], a["doppler"], a["mag"] = f + frame0, r, d, grid[f, r, d]
    return a


# ---- lists at the tile edges of the frame index ----
TILE_EDGE_CFG = Cfg(n_range=64, n_doppler=32, v_max=3 * 32 * 8, step=3)   # K = 3, one stream


def tile_edge_list(n):
    """Exactly n records of 64 x 32 frames whose last record is in frame 3: unfolded as 6 scans (two
    dwells), frames 4 and 5 are empty."""
    recs = thin_to(random_list(41, 4, 64, 32, n + n // 4 + 64, DET_DTYPE, cfg=TILE_EDGE_CFG, targets=20), n, n)
    assert len(recs) == n and recs["frame"][-1] == 3, (len(recs), n, int(recs["frame"][-1]))
    return recs


# ---- the scenario's fighter ----
TRUTH_MPS = -synth.TAC_MACH_MPS
F0_HZ = 1000.0
# (qualifying dwells, those in which the fighter's report is within one out_unit of the truth)
FIGHTER_FACT = {"sea-128x32": ([0, 6], [0, 6]), "sea-256x64": ([0, 6], [0])}


def scenario_cfg(scene):
    """K 3, step 1, the default tolerances and m_of, v_max 2 Nc 8, out_unit 8."""
    return Cfg(n_range=scene.ns, n_doppler=scene.nc, step=1, v_max=2 * scene.nc * 8)


def truth_fine(scene):
    return 2.0 * TRUTH_MPS / synth.TAC_WAVELENGTH / (F0_HZ / scene.nc)


def fighter_fact(scene, plots, vplots):
    """(qualifying dwells, dwells in which the fact holds, the fighter's report per qualifying dwell).
    A dwell qualifies when it touches no notch scan and each of its three scans holds a plot within one
    bin of the lead fighter's truth cell.  The fighter's report is the one of the dwell's first scan
    (pos 0) whose source plot is that scan's plot nearest the truth cell (largest mag among those within
    one bin).  The fact: its v_fine is within one out_unit (8 fine units) of the truth."""
    _, truth = S.scene_cubes(scene)
    r, d = plots["range"].astype(np.int64), plots["doppler"].astype(np.int64)

    def fighter_plot(s):
        rb, db = truth[s][0]
        dd = np.abs(d - db)
        at = np.flatnonzero((plots["frame"] == s) & (np.abs(r - rb) <= 1) & (np.minimum(dd, scene.nc - dd) <= 1))
        return int(at[np.argmax(plots["mag"][at])]) if len(at) else None
    qualifying, holds, reports = [], [], {}
    for j in range(n_dwells(scene.n_scans, 3, 1)):
        scans = range(j, j + 3)
        src = [fighter_plot(s) for s in scans]
        if any(s in scene.notch for s in scans) or None in src:
            continue
        qualifying.append(j)
        rep = vplots[(vplots["frame"] == j) & (vplots["src"] == src[0])]
        assert len(rep) == 1 and int(rep["pos"][0]) == 0, (j, rep)
        reports[j] = rep[0]
        if abs(int(rep["v_fine"][0]) - truth_fine(scene)) <= 8:
            holds.append(j)
    return qualifying, holds, reports
