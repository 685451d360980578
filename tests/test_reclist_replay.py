"""The record-list layer (csrc/rec_window.hpp, csrc/unfold_window.hpp) on the CPU: tools/reclist_replay.cpp,
built host-only with AddressSanitizer and UBSan by tools/reclist_replay.sh, replays the launches of the plot
extractor, the beam merger and the velocity unfolder serially over heap buffers of exactly the size the
shipped code may touch.  One child process per case; a non-empty stderr or a non-zero exit fails the test.

Well-formed lists and the limits are compared with plots_ref / merge_ref / unfold_ref by the comparison
functions of the GPU tests, status words included.  Malformed lists (the specification leaves their output
open) are held to the safety promises only: the sanitizers stay silent, the program ends, every rank
written is below out_cap (checked in the program's record writer), status[0] is the number of set mask
bits, status[1] is found - n, and no slot at or beyond min(status[0], out_cap) is written.  They are fed
to no GPU.  One of them damages not the list but the frame index the replay has just built.

Times on the CPU machine this was written on (8 CPUs), sanitizers on: a child takes 32 to 41 ms whatever the
case (the start of the sanitized program dominates; 3700 records at windows of 4: 35 ms), and 76 ms (median) to
100 ms (worst of 120) with every CPU oversubscribed twice; CHILD_TIMEOUT is five times that worst.  The build
takes 2 s.  The file takes about two minutes: some 2400 children, and the NumPy / Python references.
"""
import itertools
import os
import subprocess

import numpy as np
import pytest

import reclist_cases as RC
from conftest import REPO
from fmcw import DET_DTYPE, MPLOT_DTYPE, PLOT_DTYPE, VPLOT_DTYPE
from gpu_support import GUARD, SENTINEL
from merge_ref import assert_mplots_match, merge_ref, random_list as merge_list, tile_edge_list
from plots_ref import assert_plots_match, plots_ref
from tile_edge import TILE_EDGE_SIZES
from unfold_ref import Cfg, assert_vplots_equal, random_list as unfold_list, unfold_ref

CHILD_TIMEOUT = 0.5
PLOTS, MERGE, UNFOLD = 0, 1, 2
OUT_DTYPE = {PLOTS: PLOT_DTYPE, MERGE: MPLOT_DTYPE, UNFOLD: VPLOT_DTYPE}


class Replay:
    def __init__(self, exe, tmp):
        self.exe, self.tmp, self.runs = exe, tmp, 0

    def __call__(self, obj, recs, cfg_words, n_arg=0, max_groups=0, out_cap=None, rec_cap=None, max_recs=None,
                 n_word=None, per_rec=1, index_damage=0):
        """One call of object `obj` on a host list: (status words, records written, the sentinel-filled
        output buffer's bytes after them, set mask bits)."""
        n, stride = len(recs), recs.dtype.itemsize
        rec_cap = n if rec_cap is None else rec_cap
        max_recs = max(n, 1) if max_recs is None else max_recs
        out_cap = max(per_rec * n, 1) if out_cap is None else out_cap
        raw = np.ascontiguousarray(recs).tobytes()
        head = np.zeros(40, "<u4")
        head[:10] = [0x50524C52, obj, stride, rec_cap, max_recs, n if n_word is None else n_word, n_arg, out_cap, len(raw),
                     max_groups]
        head[10:10 + len(cfg_words)] = cfg_words
        head[39] = index_damage
        case, result = self.tmp / "case.bin", self.tmp / "result.bin"
        case.write_bytes(head.tobytes() + raw)
        result.unlink(missing_ok=True)
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
        p = subprocess.run([str(self.exe), str(case), str(result)], capture_output=True, text=True, timeout=CHILD_TIMEOUT, env=env)
        self.runs += 1
        if p.returncode or p.stderr:
            print(p.stderr)
            pytest.fail(f"reclist_replay: exit {p.returncode}, {len(p.stderr)} bytes on stderr (printed above)")
        out = np.frombuffer(result.read_bytes(), np.uint8)
        r = out[:32].view("<u4")
        assert r[0] == 0x53524C52 and r[1] == 2 + obj and r[7] == out_cap and len(out) == 32 + 32 * out_cap
        status = [int(x) for x in r[2:2 + r[1]]]
        assert all(int(x) == GUARD for x in r[2 + r[1]:6]), "a status word the object does not have was written"
        k = min(status[0], out_cap)
        slots = out[32:]
        return status, slots[:k * 32].view(OUT_DTYPE[obj]).copy(), slots[k * 32:], int(r[6])


@pytest.fixture(scope="module")
def replay(tmp_path_factory):
    d = tmp_path_factory.mktemp("reclist_replay")
    p = subprocess.run(["bash", str(REPO / "tools" / "reclist_replay.sh"), "-o", str(d)], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and (d / "reclist_replay").exists(), p.stdout + p.stderr
    return Replay(d / "reclist_replay", d)


def dets_list(seed, nf, nr, nd, density, levels=5):
    a = merge_list(seed, nf, nr, nd, density, DET_DTYPE, levels)
    a["threshold"] = np.random.default_rng(seed).random(len(a)).astype(np.float32)
    return a


def as_stride(recs, stride):
    """The list's frame / range / doppler / mag in records of `stride` bytes."""
    out = np.zeros(len(recs), DET_DTYPE if stride == 16 else PLOT_DTYPE)
    for name in ("frame", "range", "doppler", "mag"):
        out[name] = recs[name]
    return out


def check_plots(replay, dets, nr, nd, win, out_cap=None, rec_cap=None, max_recs=None, n_word=None):
    n = len(dets)
    cut = min(n if rec_cap is None else rec_cap, max(n, 1) if max_recs is None else max_recs)
    want = plots_ref(dets[:cut], nr, nd, *win)
    st, got, rest, bits = replay(PLOTS, dets, [nr, nd, *win], out_cap=out_cap, rec_cap=rec_cap, max_recs=max_recs, n_word=n_word)
    found = n if n_word is None else n_word
    assert st == [len(want), found - min(found, cut)] and bits == len(want), (st, len(want), bits)
    assert_plots_match(got, want[:len(got)])
    assert len(got) == (len(want) if out_cap is None else min(len(want), out_cap))
    assert np.all(rest == SENTINEL)
    return want


def check_merge(replay, recs, nr, nd, nb, win, wrap=False, n_maps=None, out_cap=None, rec_cap=None, max_recs=None,
                n_word=None):
    n = len(recs)
    if n_maps is None:
        n_maps = (int(recs["frame"].max()) // nb + 1) * nb if n else nb
    cut = min(n if rec_cap is None else rec_cap, max(n, 1) if max_recs is None else max_recs)
    want, beyond = merge_ref(recs[:cut], nr, nd, nb, win, wrap, n_maps)
    st, got, rest, bits = replay(MERGE, recs, [nr, nd, nb, *win, int(wrap)], n_arg=n_maps, max_groups=max(n_maps, nb),
                                 out_cap=out_cap, rec_cap=rec_cap, max_recs=max_recs, n_word=n_word)
    found = n if n_word is None else n_word
    assert st == [len(want), found - min(found, cut), beyond] and bits == len(want), (st, len(want), beyond, bits)
    assert len(got) == (len(want) if out_cap is None else min(len(want), out_cap))
    assert_mplots_match(got, want[:len(got)], win)
    assert np.all(rest == SENTINEL)
    return want


def unfold_words(c: Cfg):
    return [c.n_range, c.n_doppler, c.n_prf, *c.prf_units, *([0] * (8 - c.n_prf)), c.prf_phase, c.step, c.zero_bin, c.v_max,
            c.out_unit, c.tol_range, c.tol_doppler, c.m_of, c.n_streams]


def check_unfold(replay, recs, n_scans, cfg, out_cap=None, rec_cap=None, max_recs=None, n_word=None, max_frames=None):
    n = len(recs)
    cut = min(n if rec_cap is None else rec_cap, max(n, 1) if max_recs is None else max_recs)
    want, beyond, tied = unfold_ref(recs[:cut], n_scans, cfg)
    st, got, rest, bits = replay(UNFOLD, recs, unfold_words(cfg), n_arg=n_scans,
                                 max_groups=max(n_scans, 1) * cfg.n_streams if max_frames is None else max_frames,
                                 out_cap=out_cap, rec_cap=rec_cap, max_recs=max_recs, n_word=n_word, per_rec=cfg.n_prf)
    found = n if n_word is None else n_word
    assert st == [len(want), found - min(found, cut), beyond, tied] and bits == len(want), (st, len(want), beyond, tied, bits)
    assert len(got) == (len(want) if out_cap is None else min(len(want), out_cap))
    assert_vplots_equal(got, want[:len(got)])
    assert np.all(rest == SENTINEL)
    return want


# ---- 3a: well-formed lists, record for record ----------------------------------------------------------
MAPS = [(8, 8), (16, 9), (32, 32)]          # 16 x 9: n_doppler == 2 win_doppler + 1 at win_doppler 4
DENSITIES = [0.05, 0.5, 1.0]
BEAM_TRIPLES = [(wb, nb, wrap, stride) for wb in (0, 1, 4) for nb in (1, 2, 3, 8, 9) for wrap in (False, True)
                for stride in (16, 32) if not wrap or nb >= 2 * wb + 1]


@pytest.mark.parametrize("density", DENSITIES)
@pytest.mark.parametrize("nr,nd", MAPS)
def test_plots_and_merge_over_every_window(replay, nr, nd, density):
    """Every (win_range, win_doppler) in 0..4 x 0..4 that the map admits: the plot extractor on 3 frames, and the
    merger with one (win_beam, n_beams, wrap, stride) of BEAM_TRIPLES per window, in turn, so that over the
    nine (map, density) cases every admitted combination of win_beam 0 / 1 / 4, n_beams 1 / 2 / 3 / 8 / 9, wrap
    on / off and stride 16 / 32 runs about four times.  Two scans (one on 32 x 32)."""
    dets = dets_list(100 + nr, 3, nr, nd, density)
    scans = 1 if nr == 32 else 2
    turn = (MAPS.index((nr, nd)) * 3 + DENSITIES.index(density)) * 25
    plots = merged = 0
    lists = {}
    for wr, wd in itertools.product(range(5), range(5)):
        if nd < 2 * wd + 1:
            continue
        plots += len(check_plots(replay, dets, nr, nd, (wr, wd)))
        wb, nb, wrap, stride = BEAM_TRIPLES[turn % len(BEAM_TRIPLES)]
        turn += 1
        if (nb, stride) not in lists:
            lists[nb, stride] = as_stride(merge_list(200 + nb, scans * nb, nr, nd, density), stride)
        merged += len(check_merge(replay, lists[nb, stride], nr, nd, nb, (wb, wr, wd), wrap))
    assert plots > 0 and merged > 0


def test_every_beam_combination_runs():
    """The turn-taking above reaches every entry of BEAM_TRIPLES."""
    seen = set()
    for k, (nr, nd) in enumerate(MAPS):
        for j in range(3):
            turn = (k * 3 + j) * 25
            for wr, wd in itertools.product(range(5), range(5)):
                if nd >= 2 * wd + 1:
                    seen.add(turn % len(BEAM_TRIPLES))
                    turn += 1
    assert seen == set(range(len(BEAM_TRIPLES)))


def test_ties_go_to_the_first_in_list_order(replay):
    """Equal magnitudes over whole windows: full 16 x 9 maps of ones.  Every cell but a frame's first has an equal
    record before it in its window (not a peak itself, but that is not asked), so each frame, and with three
    beams each scan, reports its first cell alone."""
    dets = dets_list(7, 2, 16, 9, 1.0, levels=1)
    want = check_plots(replay, dets, 16, 9, (4, 4))
    assert [(int(p["frame"]), int(p["range"]), int(p["doppler"])) for p in want] == [(0, 0, 0), (1, 0, 0)]
    recs = merge_list(8, 6, 16, 9, 1.0, levels=1)
    for wrap in (False, True):
        want = check_merge(replay, recs, 16, 9, 3, (1, 4, 4), wrap)
        assert [tuple(int(p[k]) for k in ("frame", "beam", "range", "doppler")) for p in want] == [(0, 0, 0, 0), (1, 0, 0, 0)]


@pytest.mark.parametrize("n", TILE_EDGE_SIZES)
def test_lists_at_the_tile_edge(replay, n):
    recs = tile_edge_list(n)
    assert len(check_merge(replay, recs, 32, 32, 3, (1, 1, 1), False, n_maps=6)) > 0
    assert len(check_merge(replay, as_stride(recs, 32), 32, 32, 3, (1, 2, 4), True, n_maps=6)) > 0
    dets = recs.copy()
    dets["threshold"] = 0.5 * dets["mag"]
    assert len(check_plots(replay, dets, 32, 32, (1, 1))) > 0
    assert len(check_plots(replay, dets, 32, 32, (4, 4))) > 0


@pytest.mark.parametrize("win", [(1, 1, 1), (1, 4, 4)])
def test_maps_straddle_both_tile_edges_and_the_halo(replay, win):
    """2 beams x 64 x 32 at density 0.9: about 1840 records per map, 3700 in all (above 2 tiles + halo).  Map 0
    straddles record 1024 and map 1 record 2048, and a record's neighbours in the other beam lie a whole map,
    more than the 512-record halo, away: staged and in-place probes on both sides of both halo edges."""
    recs = merge_list(34, 2, 64, 32, 0.9)
    per_map = np.bincount(recs["frame"], minlength=2)
    assert per_map[0] > 1024 + 512 and per_map[0] < 2048 < len(recs) and len(recs) > 2 * 1024 + 512
    check_merge(replay, recs, 64, 32, 2, win, False)
    dets = recs.copy()
    dets["threshold"] = 0.25
    check_plots(replay, dets, 64, 32, win[1:])


def test_n_maps_suffix_empty_maps_and_the_empty_list(replay):
    recs = merge_list(38, 9, 32, 16, 0.4)
    for n_maps in (0, 3, 6, 9):
        want = check_merge(replay, recs, 32, 16, 3, (1, 1, 1), True, n_maps=n_maps)
        assert (len(want) > 0) == (n_maps > 0)
    # beams 1 and 3 of scan 0 and the whole of scan 1 hold no record; then a leading gap of four maps
    recs = merge_list(39, 15, 32, 16, 0.4)
    holes = recs[~np.isin(recs["frame"], [1, 3, 5, 6, 7, 8, 9])]
    for wrap in (False, True):
        check_merge(replay, holes, 32, 16, 5, (2, 1, 1), wrap, n_maps=15)
    check_merge(replay, holes[holes["frame"] >= 4], 32, 16, 5, (1, 1, 1), True, n_maps=15)
    for stride_list in (np.zeros(0, DET_DTYPE), np.zeros(0, PLOT_DTYPE)):
        check_merge(replay, stride_list, 32, 16, 3, (1, 1, 1), n_maps=6, out_cap=8)
        check_merge(replay, stride_list, 32, 16, 3, (1, 1, 1), n_maps=6, out_cap=8, n_word=7)   # a zero rec_cap
    check_plots(replay, np.zeros(0, DET_DTYPE), 32, 16, (1, 1), out_cap=8)
    check_plots(replay, np.zeros(0, DET_DTYPE), 32, 16, (1, 1), out_cap=8, n_word=7)
    st, got, rest, bits = replay(PLOTS, dets_list(1, 2, 32, 16, 0.3), [32, 16, 1, 1], n_word=0)   # records, a zero count
    assert st == [0, 0] and bits == 0 and np.all(rest == SENTINEL)


def test_caps(replay):
    """rec_cap and max_recs below the count word, out_cap below the number of reports and 0."""
    recs = merge_list(37, 6, 32, 32, 0.4)
    dets = dets_list(14, 3, 32, 32, 0.4)
    n, m = len(recs), len(dets)
    assert n > 2048 and m > 1024
    check_merge(replay, recs, 32, 32, 3, (1, 1, 1), n_maps=6, rec_cap=n - 700, n_word=n + 5)
    check_merge(replay, recs, 32, 32, 3, (1, 1, 1), n_maps=6, max_recs=1500)
    check_plots(replay, dets, 32, 32, (1, 1), rec_cap=m - 300, n_word=m + 5)
    check_plots(replay, dets, 32, 32, (1, 1), max_recs=1100)
    for cap in (0, 1, 40):
        want = check_merge(replay, recs, 32, 32, 3, (1, 1, 1), n_maps=6, out_cap=cap)
        assert len(want) > 3 * 40                       # the cap falls inside the first of three tiles
        assert len(check_plots(replay, dets, 32, 32, (1, 1), out_cap=cap)) > 40
    ucfg = Cfg(n_range=32, n_doppler=16, v_max=3 * 16 * 8, step=1)
    urecs = unfold_list(3, 9, 32, 16, 1300, PLOT_DTYPE, cfg=ucfg, targets=20)
    assert len(urecs) > 1024
    check_unfold(replay, urecs, 9, ucfg, rec_cap=len(urecs) - 300, n_word=len(urecs) + 5)
    check_unfold(replay, urecs, 9, ucfg, max_recs=700)
    for cap in (0, 1, 40):
        assert len(check_unfold(replay, urecs, 9, ucfg, out_cap=cap)) > 40


UNITS = (7, 8, 9, 11, 13, 15, 16, 17)        # pairwise distinct; K PRFs are its first K
U_NR, U_NC = 16, 16
# (zero_bin, tolerance, v_max as a multiple of Nc p_min, out_unit 1 or the largest, stride): 108 combinations
U_REST = list(itertools.product((0, U_NC // 2, U_NC - 1), (0, 2, 4), (0, 3, 32), (False, True), (16, 32)))


def unfold_configs():
    """(K, step, m_of, n_streams, prf_phase) in full, K 2..8, step 1 / between / K, m_of 1 / K - 1 / K, streams
    1 / 2 / 3, every phase: 915 of them, each with one entry of U_REST in turn (two for one stream): 1220."""
    out, turn = [], 0
    for K in range(2, 9):
        for step in sorted({1, (K + 1) // 2, K}):
            for m_of in sorted({1, K - 1, K}):
                for ns in (1, 2, 3):
                    for phase in range(K):
                        for _ in range(2 if ns == 1 else 1):
                            out.append((K, step, m_of, ns, phase, *U_REST[(turn * 37) % len(U_REST)]))   # 37: coprime to 108
                            turn += 1
    return out


U_CONFIGS = unfold_configs()


def unfold_case(k, K, step, m_of, ns, phase, zb, tol, vm, big_unit, stride):
    p = UNITS[:K]
    v_max = vm * U_NC * min(p)
    cfg = Cfg(n_range=U_NR, n_doppler=U_NC, prf_units=p, prf_phase=phase, step=step, zero_bin=zb, v_max=v_max,
              out_unit=65535 if big_unit else 1, tol_range=tol, tol_doppler=tol, m_of=m_of, n_streams=ns)
    n_scans = K + step                                    # two dwells, and one frame beyond the last scan
    # the Python reference looks at hypotheses x K x window cells for each (dwell, record) pair: fewer records
    # where that is large
    cost = (2 * vm + 1) * K * (2 * tol + 1) ** 2 * -(-K // step)
    clutter = int(np.clip(150000 // cost, 6, 60))
    recs = unfold_list(5000 + k, n_scans * ns + 1, U_NR, U_NC, clutter, DET_DTYPE if stride == 16 else PLOT_DTYPE,
                       levels=3, targets=2 if cost < 10000 else 1, cfg=cfg)
    return cfg, n_scans, recs


def test_unfold_configurations_cover_the_table():
    assert len(U_CONFIGS) >= 1152 and len(set(U_CONFIGS)) == len(U_CONFIGS)
    for col, values in ((0, range(2, 9)), (3, (1, 2, 3)), (5, (0, 8, 15)), (6, (0, 2, 4)), (7, (0, 3, 32)), (8, (False, True)),
                        (9, (16, 32))):
        for K in range(2, 9):
            assert {c[col] for c in U_CONFIGS if c[0] == K} == ({K} if col == 0 else set(values)), (col, K)
    for K in range(2, 9):
        assert {(c[1], c[2], c[4]) for c in U_CONFIGS if c[0] == K} == set(
            itertools.product({1, (K + 1) // 2, K}, {1, K - 1, K}, range(K)))


@pytest.mark.parametrize("K", range(2, 9))
def test_unfold_configurations(replay, K):
    reports, full = 0, 0
    for k, c in enumerate(U_CONFIGS):
        if c[0] != K:
            continue
        cfg, n_scans, recs = unfold_case(k, *c)
        want = check_unfold(replay, recs, n_scans, cfg)
        reports += len(want)
        full += int((want["n_hits"] == K).sum())
        if K > 4:
            assert not len(want) or want["hit_mask"].max() < (1 << K)
    assert reports > 0 and full > 0, (reports, full)
    if K > 4:
        cfg, n_scans, recs = unfold_case(0, K, K, 2, 1, 0, 0, 2, 3, False, 32)
        want = check_unfold(replay, recs, n_scans, cfg)
        assert (want["hit_mask"] >> 4).any()


def test_unfold_too_few_scans_and_frames_beyond(replay):
    cfg = Cfg(n_range=U_NR, n_doppler=U_NC, prf_units=UNITS[:5], v_max=3 * U_NC * 7, step=2, n_streams=2, m_of=2, out_unit=7)
    recs = unfold_list(6, 9 * 2, U_NR, U_NC, 200, DET_DTYPE, cfg=cfg)
    for n_scans in (0, 1, 4, 5, 6, 7, 9):
        want = check_unfold(replay, recs, n_scans, cfg)
        assert (len(want) > 0) == (n_scans >= 5)
    for n_word in (None, 7):
        check_unfold(replay, np.zeros(0, PLOT_DTYPE), 9, cfg, out_cap=8, n_word=n_word)


# ---- 3b: the limits --------------------------------------------------------------------------------------
def test_limits_plots_and_merge(replay):
    """n_range = n_doppler = 65536, records at (0, 0), (0, 65535), (65535, 0), (65535, 65535) and their neighbours
    across the Doppler wrap, windows of 4."""
    dets = RC.corner_list(3, DET_DTYPE)
    want = check_plots(replay, dets, RC.LIMIT, RC.LIMIT, RC.PLOTS_CORNER_WIN)
    assert 0 < len(want) < len(dets) and want["n_cells"].max() > 4
    m = RC.MERGE_CORNER
    for stride, wrap in itertools.product((16, 32), (False, True)):
        recs = RC.corner_list(m["n_maps"] + 1, DET_DTYPE if stride == 16 else PLOT_DTYPE, seed=stride)
        want = check_merge(replay, recs, RC.LIMIT, RC.LIMIT, m["n_beams"], m["win"], wrap, n_maps=m["n_maps"])
        assert 0 < len(want) and want["n_merged"].max() > 8


def test_limits_unfold(replay):
    """The same corners over 5 scans at K = 3 with PRF units 4096, 4095 and 4093, tolerances of 4, zero_bin 65535
    and a v_max within 2^17 of 2^31."""
    for dtype in (DET_DTYPE, PLOT_DTYPE):
        want = check_unfold(replay, RC.unfold_corner_list(dtype), RC.UNFOLD_CORNER_SCANS, RC.UNFOLD_CORNER_CFG)
        assert (want["n_hits"] == 3).sum() >= 4 and np.abs(want["v_fine"].astype(np.int64)).max() > 2 ** 31 - 2 ** 17


def test_unfold_v_max_limit_hypotheses(replay):
    """K = 3 at the admitted v_max limit 32 Nc p_min on 32 x 32 x 8: 65 hypotheses per record."""
    cfg, recs = RC.unfold_v_max_limit_case()
    want = check_unfold(replay, recs, 8, cfg)
    assert len(want) > 0 and want["n_ties"].max() > 1 and np.abs(want["fold"]).max() >= 16


# ---- 3c: malformed lists (CPU only) ----------------------------------------------------------------------
def damage(recs, kind, n_groups, nr, nd, rng):
    a = recs.copy()
    n = len(a)
    pick = rng.choice(n, max(n // 8, 3), replace=False)
    if kind == "shuffle":
        rng.shuffle(a)
    elif kind == "duplicates":
        a[pick] = a[(pick + 1) % n]
    elif kind == "frames":
        a["frame"][pick] = rng.integers(n_groups, n_groups + 3, len(pick))
        a["frame"][pick[0]] = 0xFFFFFFFF
        a["frame"][pick[1]] = n_groups
    elif kind == "cells":
        a["range"][pick[::2]] = rng.integers(nr, 65536, len(pick[::2]))
        a["doppler"][pick[1::2]] = rng.integers(nd, 65536, len(pick[1::2]))
        a["range"][pick[0]], a["doppler"][pick[1]] = 65535, 65535
    elif kind == "mags":
        a["mag"][pick] = rng.choice(np.array([np.nan, np.inf, -np.inf], np.float32), len(pick))
    return a


DAMAGE = ["shuffle", "duplicates", "frames", "cells", "mags", "count_word", "everything", "index"]


def malformed(replay, obj, recs, words, kind, n_groups, nr, nd, seed, **kw):
    rng = np.random.default_rng(seed)
    kinds = ["shuffle", "duplicates", "frames", "cells", "mags"] if kind == "everything" else [kind]
    for k in kinds:
        recs = damage(recs, k, max(n_groups, 1), nr, nd, rng)
    n = len(recs)
    n_word = n + 1000 if kind in ("count_word", "everything") else n
    if kind == "index" and obj != PLOTS:      # words of start[] far above the list's length (the program's case word 39)
        kw["index_damage"] = 2 + seed % 2
    for out_cap in (None, 5)[:1 + seed % 2]:
        st, got, rest, bits = replay(obj, recs, words, out_cap=out_cap, n_word=n_word, **kw)
        assert st[0] == bits and st[1] == n_word - n, (kind, st, bits)
        assert np.all(rest == SENTINEL), kind


@pytest.mark.parametrize("kind", DAMAGE)
def test_malformed_lists(replay, kind):
    """3a's lists, damaged: shuffled, cells listed twice, frames at or above n_groups in the middle (one of them
    0xffffffff), range >= n_range / doppler >= n_doppler, NaN and +-Inf magnitudes, a count word above
    rec_cap, and all of it at once.  "index": the list is sound, but every second or third word of the frame
    index is far above the list's length, which segment() has to clip (a freshly built index never asks that
    of it: its last word is its largest)."""
    seed = DAMAGE.index(kind)
    for nr, nd, density in ((8, 8, 0.5), (16, 9, 1.0), (32, 32, 0.5)):
        wins = [(0, 0), (1, 1), (4, min(4, (nd - 1) // 2))]
        dets = dets_list(100 + nr, 3, nr, nd, density)
        for win in wins:
            malformed(replay, PLOTS, dets, [nr, nd, *win], kind, 3, nr, nd, seed)
        for wb, nb, wrap, stride in BEAM_TRIPLES[seed::14]:
            recs = as_stride(merge_list(200 + nb, 2 * nb, nr, nd, density), stride)
            for wr, wd in wins:
                malformed(replay, MERGE, recs, [nr, nd, nb, wb, wr, wd, int(wrap)], kind, 2 * nb, nr, nd, seed, n_arg=2 * nb,
                          max_groups=2 * nb)
    recs = merge_list(34, 2, 64, 32, 0.9)                       # three tiles, staged and in-place probes
    malformed(replay, MERGE, recs, [64, 32, 2, 1, 4, 4, 0], kind, 2, 64, 32, seed, n_arg=2, max_groups=2)
    for k, c in list(enumerate(U_CONFIGS))[seed::47]:
        cfg, n_scans, recs = unfold_case(k, *c)
        malformed(replay, UNFOLD, recs, unfold_words(cfg), kind, n_scans * cfg.n_streams, U_NR, U_NC, seed, n_arg=n_scans,
                  max_groups=n_scans * cfg.n_streams, per_rec=cfg.n_prf)
    ucfg = Cfg(n_range=32, n_doppler=16, v_max=3 * 16 * 8, step=1)
    urecs = unfold_list(3, 9, 32, 16, 1300, PLOT_DTYPE, cfg=ucfg, targets=20)     # two tiles of records, six of pairs
    malformed(replay, UNFOLD, urecs, unfold_words(ucfg), kind, 9, 32, 16, seed, n_arg=9, max_groups=9, per_rec=3)
