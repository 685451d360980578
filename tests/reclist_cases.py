"""Record lists at the limits the create checks admit (n_range = n_doppler = 65536, windows of 4, PRF units
of 4096), shared by test_reclist_replay.py (the list layer on the CPU under sanitizers) and the GPU tests
of the plot extractor, the beam merger and the velocity unfolder.  A helper, not a test module.

The objects take only the list, so a 65536 x 65536 map costs nothing: max_recs is the list's length.
"""
import numpy as np

from unfold_ref import Cfg, predicted_bin

LIMIT = 65536
TOP = LIMIT - 1
# the four corners and their neighbours: across the Doppler wrap (columns 65535 and 0 are neighbours), along
# the clamped range axis (rows 0 and 65535 are not), and cells 4 away, at the rim of the widest window
CORNER_CELLS = sorted({(r, d) for r0 in (0, TOP) for d0 in (0, TOP)
                       for dr, dd in ((0, 0), (0, 1), (1, 0), (1, 1), (0, -1), (1, -1), (0, 4), (4, 0), (4, -4), (0, -4),
                                      (3, 5), (5, 0))
                       for r in [r0 + dr if r0 == 0 else r0 - dr] for d in [(d0 + dd) % LIMIT]})


def corner_list(n_frames, dtype, seed=0, drop=0.25):
    """CORNER_CELLS in each of n_frames frames, a quarter of them left out per frame, magnitudes from {1..4}
    (ties across the wrap); the four corners themselves are in every frame."""
    rng = np.random.default_rng(1000 + seed)
    rows = []
    for f in range(n_frames):
        for r, d in CORNER_CELLS:
            corner = r in (0, TOP) and d in (0, TOP)
            if corner or rng.random() >= drop:
                rows.append((f, r, d, float(rng.integers(1, 5))))
    a = np.zeros(len(rows), dtype)
    for i, (f, r, d, m) in enumerate(sorted(rows)):
        a["frame"][i], a["range"][i], a["doppler"][i], a["mag"][i] = f, r, d, m
    if "threshold" in (dtype.names or ()):
        a["threshold"] = rng.random(len(a)).astype(np.float32)
    return a


PLOTS_CORNER_WIN = (4, 4)
MERGE_CORNER = dict(n_beams=9, win=(4, 4, 4), n_maps=18)       # 2 scans x 9 beams (2 win_beam + 1), wrapped and clamped

# K = 3 at the largest PRF units; v_max is the largest value the out_unit check admits at out_unit 65535
# (below the 32 n_doppler p_min of the v_max check), so v + v_max comes within 2^17 of 2^32
UNFOLD_CORNER_CFG = Cfg(n_range=LIMIT, n_doppler=LIMIT, prf_units=(4096, 4095, 4093), prf_phase=1, step=1, zero_bin=TOP,
                        v_max=65534 * 65535 // 2, out_unit=65535, tol_range=4, tol_doppler=4, m_of=2, n_streams=1)
UNFOLD_CORNER_SCANS = 5


def unfold_corner_list(dtype):
    """corner_list over 5 scans (and one frame beyond them) plus movers in rows 0, 65535 and 4 written where
    their velocity folds to at each scan's PRF, one of them at v_max."""
    cfg = UNFOLD_CORNER_CFG
    a = corner_list(UNFOLD_CORNER_SCANS + 1, dtype, seed=7)
    cells = {(int(x["frame"]), int(x["range"]), int(x["doppler"])): float(x["mag"]) for x in a}
    for r, v in ((0, cfg.v_max), (TOP, -cfg.v_max + 12345), (4, 987654321), (TOP - 4, -40000)):
        for s in range(UNFOLD_CORNER_SCANS):
            p = cfg.prf_units[(s + cfg.prf_phase) % cfg.n_prf]
            cells[(s, r, predicted_bin(v, p, cfg.zero_bin, LIMIT))] = 9.0
    out = np.zeros(len(cells), dtype)
    for i, ((f, r, d), m) in enumerate(sorted(cells.items())):
        out["frame"][i], out["range"][i], out["doppler"][i], out["mag"][i] = f, r, d, m
    return out


def unfold_v_max_limit_case():
    """(cfg, list): K = 3 on 8 scans of 32 x 32 at the v_max limit 32 Nc p_min, 65 hypotheses per record of the
    slowest PRF; 200-300 records with movers over the whole velocity range."""
    from fmcw import PLOT_DTYPE
    from unfold_ref import random_list
    cfg = Cfg(n_range=32, n_doppler=32, prf_units=(8, 9, 10), step=1, v_max=32 * 32 * 8, out_unit=1)
    recs = random_list(91, 8, 32, 32, 220, PLOT_DTYPE, cfg=cfg, targets=8)
    assert 200 <= len(recs) <= 300, len(recs)
    return cfg, recs
