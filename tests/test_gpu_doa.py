"""Angle resolution on the GPU (fmcw_doa_* of libfmcw.so on gfx950 through the C-ABI), every case against
tests/doa_ref.py (the specification in fp64 NumPy, forced along the GPU's picks).  The tolerances are
doa_ref.assert_doa_match's (derived there); every comparison prints the worst fraction of each bound it used.

Shapes: n_ch 1, 2, 3, 16, 64; n_grid 64 (one grid point per lane), 128 and 1024 (16 per lane, the limit);
k_max 1 and 4, relax_passes 0 and 2, refine on and off.  The parabola is compared where doa_ref calls it
conditioned; tests/test_doa_host.py shows on the reference alone that the cases with refine on skip at most
5 % of their sources, which is why the small arrays and the 1024-point grid refine with one source only.
"""
import numpy as np
import pytest

from fmcw import (BEARING_DTYPE, DET_DTYPE, DOA_DTYPE, AngleResolver, BearingEstimator, DeviceBuffer, FmcwError,
                  RadarCore, VirtualArray, line_steering, synth)
import doa_ref as D
from gpu_support import SENTINEL, Hip, assert_all_written, assert_sentinel_after, sentinel_buffer

pytestmark = pytest.mark.gpu


def run(ar, snaps, cells=None, rec_cap=None, n_word=None, spectrum=True):
    """One fmcw_doa_enqueue on host data into sentinel-filled buffers with 4 slots to spare.  Returns
    (status words, DOA_DTYPE records written, float32 spectrum rows written or None) after checking that
    nothing was stored beyond record n and that every word before it was."""
    n, nch, ng = len(snaps), ar.cfg.n_ch, ar.cfg.n_grid
    rec_cap = n if rec_cap is None else rec_cap
    slots = max(n, rec_cap) + 4
    bufs = []
    try:
        dsn = DeviceBuffer(max(snaps.nbytes, 8))
        bufs.append(dsn)
        if n:
            dsn.upload(np.ascontiguousarray(snaps, np.complex64))
        dc = None
        if cells is not None:
            dc = DeviceBuffer(max(cells.nbytes, 8))
            bufs.append(dc)
            if n:
                dc.upload(np.ascontiguousarray(cells))
        dn = DeviceBuffer(8)
        dn.upload(np.array([n if n_word is None else n_word, 0], np.uint32))
        do = sentinel_buffer(slots * 96)
        dsp = sentinel_buffer(slots * ng * 4) if spectrum else None
        dst = sentinel_buffer(16)
        bufs += [b for b in (dn, do, dsp, dst) if b is not None]
        ar.enqueue(dsn, dc, 0 if cells is None else cells.dtype.itemsize, rec_cap, dn, do, dsp, dst.ptr + 4)
        stw = dst.download(np.uint32, (4,))
        assert stw[0] == stw[3] == 0xA5A5A5A5, stw
        st = stw[1:3]
        k = int(st[0])
        assert k <= slots - 4
        raw = do.download(np.uint8, (slots * 96,))
        assert_sentinel_after(raw, k, 96, "angle records")
        got = raw[: k * 96].view(DOA_DTYPE).copy()
        sp = None
        if spectrum:
            raw = dsp.download(np.uint8, (slots * ng * 4,))
            assert_sentinel_after(raw, k, ng * 4, "spectrum rows")
            assert_all_written(raw[: k * ng * 4], "spectrum rows")
            sp = raw[: k * ng * 4].view(np.float32).reshape(k, ng).copy()
        return st, got, sp
    finally:
        for b in bufs:
            b.free()


def check(snaps, steering, label, cells=None, **cfg):
    """The runs with relax_passes 0 .. cfg's against the reference; returns the last run's output."""
    nch = steering.shape[1]
    passes = cfg.get("relax_passes", 2)
    runs, sp = [], None
    for p in range(passes + 1):
        with AngleResolver(nch, steering, **dict(cfg, relax_passes=p)) as ar:
            st, got, sp = run(ar, snaps, cells)
        bad = sum(1 for s in snaps if not np.all(np.isfinite(s)) or not np.any(s))
        assert list(st) == [len(snaps), bad], (st, bad)
        runs.append(got)
    used = D.assert_doa_match(runs, sp, snaps, steering, cells=cells, label=label, **cfg)
    print(f"\n{label}: {len(snaps)} records, fraction of each bound used: " + ", ".join(f"{k} {v:.3g}" for k, v in used.items()))
    return runs[-1], sp


def with_dead_records(snaps):
    """Record 3 all zeros, record 7 with a NaN, record 8 with an infinity."""
    s = snaps.copy()
    s[3] = 0
    s[7, -1] = complex(np.nan, 1.0)
    s[8, 0] = complex(1.0, np.inf)
    return s


@pytest.mark.parametrize("case", D.GPU_CASES, ids=D.case_id)
def test_against_reference(gpu, case):
    """White Gaussian snapshots (every record a hard case: no dominant source, later stages near the
    min_rel limit) and planted 1-3 source snapshots, with a zero, a NaN and an infinite snapshot among
    them; cells from a BEARING_DTYPE list (stride 32) or a DET_DTYPE list (stride 16)."""
    snaps, steering, cfg = D.gpu_case(case)
    snaps = with_dead_records(snaps)
    n = len(snaps)
    cells = np.zeros(n, BEARING_DTYPE if case["n_ch"] % 2 else DET_DTYPE)
    cells["frame"], cells["range"], cells["doppler"] = np.arange(n) + 70000, np.arange(n) % 8192, (7 * np.arange(n)) % 1024
    got, sp = check(snaps, steering, D.case_id(case), cells=cells, **cfg)
    for i in (3, 7, 8):
        assert got[i]["flags"] & 1 and got[i]["n_src"] == 0 and got[i]["total"] == 0 and got[i]["residual"] == 0
        assert not np.any(sp[i]) and got[i]["src"].tobytes() == bytes(64)
    live = np.ones(n, bool)
    live[[3, 7, 8]] = False
    assert np.all(got["flags"][live] == (2 if case["n_ch"] == 1 else 0)) and np.all(got["n_src"][live] >= 1)
    if case["kind"] == "planted":
        # the strongest source of every record within one grid step of its truth
        truth = (case["nus"][0] / 0.5 + 1.0) * case["n_grid"] / 2.0
        assert np.all(np.abs(got["src"]["pos"][live, 0] - truth) <= 1.0)


@pytest.mark.parametrize("n_ch,n_grid,k_max,relax", [(16, 128, 2, 2), (64, 1024, 4, 0), (3, 64, 1, 0)])
def test_lists_and_grids(gpu, n_ch, n_grid, k_max, relax):
    """Lists of 0, 1, 5 and 301 records at 1, 3 and the built-in number of workgroups: the same bytes
    under every grid (with 1 workgroup a wave goes round its loop 76 times, with 3 workgroups 26 times: 12
    does not divide 301), count words above and below the list, and nothing stored beyond record n."""
    steering, _ = D.line_table(n_ch, n_grid)
    snaps = D.white(301, n_ch, 99)
    with AngleResolver(n_ch, steering, k_max=k_max, relax_passes=relax) as ar:
        for n in (0, 1, 5, 301):
            base = None
            for grid in (0, 1, 3):
                ar.set_grid_for_test(grid)
                st, got, sp = run(ar, snaps[:n])
                assert list(st) == [n, 0]
                if base is None:
                    base = (got.tobytes(), sp.tobytes())
                assert (got.tobytes(), sp.tobytes()) == base, (n, grid)
            full = base
        ar.set_grid_for_test(3)
        for n_word, cap in ((400, 17), (301, 300), (0xFFFFFFFF, 22), (9, 301)):
            st, got, sp = run(ar, snaps, rec_cap=cap, n_word=n_word)
            k = min(n_word, cap)
            assert list(st) == [k, 0] and got.tobytes() == full[0][: k * 96] and sp.tobytes() == full[1][: k * n_grid * 4]
        st, got, sp = run(ar, snaps[:0], rec_cap=0, n_word=5)           # no record kernel at all
        assert list(st) == [0, 0]
        st, got, sp = run(ar, snaps, spectrum=False)
        assert sp is None and got.tobytes() == full[0]
    with AngleResolver(n_ch, steering, k_max=k_max, relax_passes=relax, max_records=10) as ar:    # max_records binds
        st, got, sp = run(ar, snaps)
        assert list(st) == [10, 0] and got.tobytes() == full[0][: 10 * 96]


def test_steering_paths(gpu):
    """The table from the host and from device memory give the same bytes; before any table no record has a
    source; a zero row and a row with a NaN are FMCW_EINVAL from the host and can never win from the
    device; a second table replaces the first."""
    n_ch, n_grid = 16, 128
    steering, _ = D.line_table(n_ch, n_grid)
    snaps = D.planted(20, n_ch, (0.10,), (1.0,), 0.01, 5)
    truth = int(round((0.10 / 0.5 + 1.0) * n_grid / 2.0))
    with AngleResolver(n_ch, steering, k_max=2) as ar:
        st, host, sp_host = run(ar, snaps)
        assert np.all(host["src"]["grid"][:, 0] == truth)
    ar = AngleResolver(n_ch, None, k_max=2, n_grid=n_grid)
    try:
        st, got, sp = run(ar, snaps)
        assert list(st) == [20, 0] and np.all(got["n_src"] == 0) and not np.any(sp) and np.all(got["total"] > 0)
        assert np.all(got["residual"] == got["total"])
        dt = DeviceBuffer(steering.nbytes)
        dt.upload(steering)
        ar.set_steering_dev(dt)
        st, dev, sp_dev = run(ar, snaps)
        assert dev.tobytes() == host.tobytes() and sp_dev.tobytes() == sp_host.tobytes()
        bad = steering.copy()
        bad[truth] = 0
        bad[truth + 1, 3] = np.nan
        for row in (truth, truth + 1):
            one = steering.copy()
            one[row] = bad[row]
            with pytest.raises(FmcwError, match=f"row {row} "):
                ar.set_steering(one)
        st, again, _ = run(ar, snaps)
        assert again.tobytes() == host.tobytes()                         # the rejected tables changed nothing
        dt.upload(bad)
        ar.set_steering_dev(dt)
        st, got, sp = run(ar, snaps)
        assert not np.any(sp[:, truth]) and not np.any(sp[:, truth + 1])
        assert np.all(got["src"]["grid"][:, 0] == truth - 1)              # the best row left
        ref = D.resolve_list(snaps, bad, k_max=2)
        assert [r["grid"][0] for r in ref] == [truth - 1] * 20
        dt.free()
        ar.set_steering(steering)
        st, got, _ = run(ar, snaps)
        assert got.tobytes() == host.tobytes()
    finally:
        ar.close()


def test_argument_checks(gpu):
    steering, _ = D.line_table(4, 64)
    with AngleResolver(4, steering) as ar:
        d = DeviceBuffer(4096)
        for stride in (0, 8, 24, 48):
            with pytest.raises(FmcwError, match="cell_stride"):
                ar.enqueue(d, d, stride, 1, d, d, None, d)
        with pytest.raises(FmcwError, match="doa_dev must be 16-byte aligned"):
            ar.enqueue(d, None, 0, 1, d, d.ptr + 8, None, d)
        with pytest.raises(FmcwError, match="null snaps_dev or doa_dev"):
            ar.enqueue(None, None, 0, 1, d, d, None, d)
        d.free()
        got, sp = ar.resolve(D.white(5, 4, 1), want_spectrum=True)
        assert len(got) == 5 and sp.shape == (5, 64)
        with pytest.raises(ValueError):
            ar.resolve(np.zeros((2, 3), np.complex64))


def test_graph_of_bearings_and_doa(gpu):
    """fmcw_bearings_enqueue -> fmcw_doa_enqueue captured into one graph on one stream (the resolver reads
    the estimator's snapshots, its records as the cells and the same count word), replayed on two lists
    of different lengths and on the first again: the reference on the snapshots the estimator wrote."""
    nf, nrx, nr, nc, cap = 2, 8, 64, 32, 64
    rng = np.random.default_rng(21)
    spec = (1000.0 * (rng.standard_normal((nf, nrx, nr, nc)) + 1j * rng.standard_normal((nf, nrx, nr, nc)))).astype(np.complex64)
    steering, _ = line_steering(nrx, 0.5, 64)
    cfg = dict(k_max=2, relax_passes=0)
    lists = []
    for n in (37, 53):
        recs = np.zeros(n, DET_DTYPE)
        recs["frame"], recs["range"], recs["doppler"] = rng.integers(0, nf, n), rng.integers(0, nr, n), rng.integers(0, nc, n)
        lists.append(recs)
    hip = Hip()
    bufs = []
    with BearingEstimator(nr, nc, nrx) as be, AngleResolver(nrx, steering, **cfg) as ar:
        try:
            dspec = DeviceBuffer(spec.nbytes)
            dspec.upload(spec)
            drec, dn = DeviceBuffer(cap * 16), DeviceBuffer(4)
            db, dsn, dst = DeviceBuffer(cap * 32), DeviceBuffer(cap * nrx * 8), DeviceBuffer(8)
            do, dsp, dst2 = DeviceBuffer(cap * 96), DeviceBuffer(cap * 64 * 4), DeviceBuffer(8)
            bufs = [dspec, drec, dn, db, dsn, dst, do, dsp, dst2]

            def calls(s):
                be.enqueue(dspec, nf, drec, 16, cap, dn, db, dsn, dst, stream=s.value)
                ar.enqueue(dsn, db, 32, cap, dn, do, dsp, dst2, stream=s.value)
            with hip.graph(calls) as (exe, s):
                seen = []
                for k in (0, 1, 0):
                    recs = lists[k]
                    drec.upload(recs)
                    dn.upload(np.array([len(recs)], np.uint32))
                    hip.replay(exe, s)
                    n = len(recs)
                    assert list(dst.download(np.uint32, (2,))) == [n, 0] == list(dst2.download(np.uint32, (2,)))
                    sn = dsn.download(np.complex64, (n, nrx))
                    got = do.download(DOA_DTYPE, (n,))
                    sp = dsp.download(np.float32, (n, 64))
                    D.assert_doa_match([got], sp, sn, steering, cells=recs, label=f"replay {k}", **cfg)
                    seen.append(got.tobytes())
                assert seen[0] == seen[2] and seen[0] != seen[1]
        finally:
            for b in bufs:
                b.free()


@pytest.mark.parametrize("n_tx,n_rx", D.CHAIN_ARRAYS)
def test_chain_two_targets_in_one_cell(gpu, n_tx, n_rx):
    """two_in_cell_frames -> fmcw_range_ct -> fmcw_mimo -> fmcw_bearings -> fmcw_doa on the GPU: the
    estimator reads one bearing more than four grid steps from either target, the resolver both within
    half a grid step (the margins of tests/test_doa_host.py on the same scene)."""
    ns, nc, cell, nus = D.CHAIN_NS, D.CHAIN_NC, D.CHAIN_CELL, D.CHAIN_NUS
    n_v, n_grid = n_tx * n_rx, D.CHAIN_GRID
    cube = np.ascontiguousarray(synth.two_in_cell_frames(1, ns, nc, n_rx, n_tx, cell=cell, rx_phase=nus, seed=D.CHAIN_SEED))
    with RadarCore(N_RANGE=ns, N_DOPPLER=nc, N_RX=n_rx, cfar="os1d", max_frames=1) as core:
        dc = DeviceBuffer(cube.nbytes)
        dc.upload(cube)
        ds = DeviceBuffer(n_rx * ns * nc * 8)
        core.range_ct(dc, ds, 1)
        with VirtualArray(ns, nc, n_rx, n_tx) as va:
            dv = DeviceBuffer(n_rx * ns * nc * 8)
            va.enqueue(ds, 1, dv)
            rec = np.zeros(1, DET_DTYPE)
            rec["range"], rec["doppler"] = cell            # cell[1] < n_d: one transmitter sees the same bin
            with BearingEstimator(ns, va.n_d, n_v, max_records=4) as be:
                bear, sn = be.estimate(dv, rec)
        for b in (dc, ds, dv):
            b.free()
    steering, st = line_steering(n_v, 0.5, n_grid)
    with AngleResolver(n_v, steering, k_max=2, relax_passes=2) as ar:
        got, _ = ar.resolve(sn, cells=bear)
    step = 0.5 * 2.0 / n_grid                                           # of nu per grid point
    assert got["n_src"][0] == 2 and (got["range"][0], got["doppler"][0]) == (cell[0], cell[1])
    est = np.sort(0.5 * (-1.0 + 2.0 * got["src"]["pos"][0, :2] / n_grid))
    print(f"\n{n_tx} TX x {n_rx} RX: phase step nu {bear['nu'][0]:.4f} (coherence {bear['coherence'][0]:.3f}), "
          f"resolver nu {est[0]:.4f} / {est[1]:.4f}, truth {nus[0]} / {nus[1]}")
    assert np.all(np.abs(est - np.sort(nus)) <= 0.5 * step)
    assert min(abs(bear["nu"][0] - nu) for nu in nus) > 4 * step
