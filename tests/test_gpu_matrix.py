"""GPU parity over the kernel test matrix (tests/kernel_matrix.py): one case per kernel variant
the dispatch tables can reach, each at the smallest shape that reaches it, against the fp64 oracle.

Tolerances are the suite's own (tests/test_gpu_parity.py): maps within 1e-4 per frame and per
significant bin (2e-3 per frame on the fp16 spectrum), detections bit-exact against the oracle CFAR
on the GPU's own map, and against the end-to-end fp64 oracle different only at near-threshold cells
(1e-4 of the threshold; on the fp16 spectrum, which misses that by its format -- worst measured
2.1e-3 -- plus the format's own per-row error bound, kernel_matrix.fp16_row_error).
The 2-D CFAR stage runs crafted maps (kernel_matrix.cfar2d_layout) at every Doppler size, strip
length, window geometry and parameter end, records bit-exact against the C oracle (the RTL-integer
oracle for compat).
The integer (RTL-compatible) datapath is an axis of its own (test_integer_path, cases
"process-int-*"): the canceller on the spectrum's 16-bit words and the integer Doppler window after
it, at every Doppler size and both cancellers, on int16 cubes that clip nowhere and on cubes that
clip at every stage.  Maps are held to the oracle's RTL arithmetic on the GPU's own range spectrum
(1e-4; AMBM plus its two floor steps), detections bit-exact, and status words 2 and 3 exactly to the
oracle's clip counts, which a second call on the same handle must reproduce.
The persistent loops (cases "*-loop-g<grid>", kernel_matrix.loops): the same cases under
fmcw_set_param's grid caps, so that a workgroup runs its loop three times and more -- the in-loop
prefetch, the LDS reuse behind the loop head's barrier, the counters over iterations, K3a's ring on
what the last strip left.  Same oracle, same bounds; then the same handle once more with the caps
at 0: map, spectrum, records and status words must be the same bytes (fmcw.h: results never depend
on tuning parameters).
The white scene (test_whole_path_every_cell, cases "*-white", kernel_matrix.WHITE): the tone scenes
above leave nearly every cell outside the targets' rows below what check_map looks at.  Every K1 / K2
key, "/loop" twins included, runs once more on white full-scale noise, where each cell is held to 1e-4
of the rms of its own range row (kernel_matrix.check_every_cell), into sentinel-filled guarded buffers.
tests/test_kernel_matrix.py shows on the CPU that the table covers the dispatch rules and that a
correct fp32 implementation passes every case that the C restatement can run.
"""
import dataclasses

import numpy as np
import pytest

import cpu_backend as CB
import fmcw_oracle as O
import kernel_matrix as K
from conftest import rel_err
from fmcw import DET_DTYPE, DeviceBuffer, RadarCore
from gpu_support import Guarded, assert_all_written, check_map, run_cfar_stage, run_range_ct

pytestmark = pytest.mark.gpu

RANGE = [c for c in K.CASES if c.group == "range"]
INTEGER = [c for c in K.CASES if c.group == "process" and c.recipe in ("int_clean", "int_sat")]
PROCESS = [c for c in K.CASES if c.group == "process" and c not in INTEGER]
CFAR1D = [c for c in K.CASES if c.group == "cfar1d"]
CFAR2D = [c for c in K.CASES if c.group == "cfar2d"]


def make_core(c: K.Cfg, nf: int, **over):
    rr, gr, rd, gd = c.cfar2d
    kw = dict(N_RANGE=c.n_range, N_DOPPLER=c.n_doppler, N_RX=c.n_rx, in_dtype=c.in_dtype, window=c.window,
              magnitude=c.magnitude, map_kind=c.map_kind, cfar=c.cfar, cfar1d=c.cfar1d,
              CFAR_REF_R=rd, CFAR_GUARD_R=gd, CFAR_REF_D=rr, CFAR_GUARD_D=gr, max_frames=nf,
              mti_bypass=c.mti == 0, NOTCH_MODE=c.mti or 2,
              compat_rtl=(("cfar",) if c.compat_cfar else ()) + (("mti",) if c.compat_mti else ()),
              range_shift=c.range_shift, spectrum=c.spectrum, cfar_rank_pct=c.cfar2d_rank_pct,
              cfar_scales=c.cfar2d_scales, cfar_scale_ovr=c.cfar2d_override)
    kw.update(over)
    return RadarCore(**kw)


GRIDS = ("grid_range", "grid_doppler", "grid_cfar2d", "grid_k3b", "grid_k3c")


def cap_grids(core, case):
    """Sets all five grid caps to case.grid (nothing for 0) and returns the created grids.  The
    mirror's iteration counts (kernel_matrix.loops) assume the cap binds: every created grid is at
    least the cap (grid_cfar2d is 0 on a handle without the 2-D CFAR)."""
    if not case.grid:
        return None
    created = {k: core.info(k) for k in GRIDS}
    print(f"{case.id}: created grids {created}, capped to {case.grid}")
    for k in GRIDS:
        core.set_param(k, case.grid)
        assert core.info(k) == min(created[k], case.grid)
        assert created[k] >= case.grid or (k == "grid_cfar2d" and case.cfg.cfar != "os2d" and created[k] == 0)
    return created


def uncap_grids(core, created):
    for k in GRIDS:
        core.set_param(k, 0)
        assert core.info(k) == created[k]


def run_stage_words(core, mag, cap):
    """fmcw_cfar: (records, the four status words)."""
    dm = DeviceBuffer(mag.nbytes)
    dm.upload(np.ascontiguousarray(mag, np.float32))
    dd = DeviceBuffer(cap * 16)
    dn = DeviceBuffer(16)
    core.cfar(dm, mag.shape[0], dd, cap, dn)
    words = dn.download(np.uint32, (4,))
    assert words[0] <= cap
    out = dd.download(DET_DTYPE, (cap,))[:int(words[0])].copy()
    for b in (dm, dd, dn):
        b.free()
    return out, [int(w) for w in words]


def same_bytes(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def same_process(a, b):
    """Two fmcw_process outputs: map bytes, records, and the status words (word 1 is 0 in both:
    fmcw_process fails on a non-zero one)."""
    same_bytes(a.rd_map, b.rd_map)
    same_bytes(a.dets, b.dets)
    assert (a.n_dets, a.window_saturations, a.word_saturations) == (b.n_dets, b.window_saturations, b.word_saturations)


@pytest.mark.parametrize("case", RANGE, ids=lambda c: c.id)
def test_range_stage(gpu, case):
    """fmcw_range_ct on white full-scale noise vs O.range_ct (fp64): 1e-4 per (frame, rx), and 1e-4
    relative on every bin above 1e-3 of that (frame, rx) peak; the K1 family is the mirror's."""
    c = case.cfg
    cube = K.make_cube(case)
    with make_core(c, case.nf) as core:
        created = cap_grids(core, case)
        got = run_range_ct(core, cube, case.nf)
        assert core.info("range_kernel") == K.range_family(c)
        if created:
            uncap_grids(core, created)
            same_bytes(run_range_ct(core, cube, case.nf), got)
    if c.window == "q15_rtl":
        ref = O.range_ct(O.window_q15_cube(cube), window=False)
    else:
        ref = O.range_ct(K.to_complex(cube, c.in_dtype))
    worst = worst_bin = 0.0
    for f in range(case.nf):
        for rx in range(c.n_rx):
            g, r = got[f, rx], ref[f, rx]
            worst = max(worst, rel_err(g, r))
            big = np.abs(r) >= 1e-3 * np.abs(r).max()
            worst_bin = max(worst_bin, float(np.max(np.abs(g[big] - r[big]) / np.abs(r[big]))))
    print(f"{case.id}: rel_err {worst:.3g}, per-bin {worst_bin:.3g}")
    assert worst <= 1e-4
    assert worst_bin <= 1e-4


def _q15_reference(core, case, cube):
    """test_process_parity's reference for the integer windows: the Doppler stage in RTL
    arithmetic on the GPU's own range spectrum (so a word's rounding is the same on both sides),
    and the fp64 end to end at frame level."""
    c = case.cfg
    spec = run_range_ct(core, cube, case.nf)
    ref = np.stack([O.magnitude(O.doppler_stage(spec[f].astype(np.complex128), mti_mode=0, q15_rtl=True), rx_axis=0)
                    for f in range(case.nf)])
    e2e = np.stack([O.process(cube[f], None, mti_mode=0, q15_rtl=True, range_shift=c.range_shift)["mag"]
                    for f in range(case.nf)])
    return ref, e2e


@pytest.mark.parametrize("case", PROCESS, ids=lambda c: c.id)
def test_whole_path(gpu, case):
    """fmcw_process: map vs the fp64 oracle, detections bit-exact vs the oracle CFAR on the GPU's
    own map (fused and stage), near-threshold rule vs the end-to-end oracle."""
    c = case.cfg
    q15 = c.window == "q15_rtl"
    if q15:
        cube = K.make_cube(case)
    else:
        cube, ref = K.reference(case)
    with make_core(c, case.nf) as core:
        created = cap_grids(core, case)
        out = core.process(cube)
        if c.map_kind == "db":
            stage = None
        else:
            stage = run_cfar_stage(core, out.rd_map, cap=out.rd_map.size)
        if q15:
            ref, e2e = _q15_reference(core, case, cube)
        if created:
            uncap_grids(core, created)
            same_process(core.process(cube), out)
            if stage is not None:
                same_bytes(run_cfar_stage(core, out.rd_map, cap=out.rd_map.size), stage)
    assert out.rd_map.shape == (case.nf, c.n_range, c.n_doppler)
    if c.map_kind == "db":
        # test_db_map: the dB map against the oracle's log of the linear map of the same input
        with make_core(c, case.nf, map_kind="linear") as core:
            created = cap_grids(core, case)
            lin = core.process(cube)
            lin_stage = run_cfar_stage(core, lin.rd_map, cap=lin.rd_map.size)
            if created:
                uncap_grids(core, created)
                same_process(core.process(cube), lin)
                same_bytes(run_cfar_stage(core, lin.rd_map, cap=lin.rd_map.size), lin_stage)
        np.testing.assert_allclose(out.rd_map, O.log_mag(lin.rd_map.astype(np.float64)), atol=2e-4)
        K.check_case_map(c, lin.rd_map, ref)
        want = K.oracle_dets(lin.rd_map, c)
        np.testing.assert_array_equal(lin.dets, want)
        np.testing.assert_array_equal(lin_stage, want)
        np.testing.assert_array_equal(out.dets, lin.dets)      # the CFAR runs on the linear values
        assert len(want) >= 1
        n, rel, frac = K.check_near_threshold(lin.dets, ref, c, case)
        print(f"{case.id}: {n} decisions differ from the fp64 end to end, worst |cut-thr|/thr {rel:.3g}, "
              f"worst gap/margin {frac:.3g}")
        return
    if q15:
        assert rel_err(out.rd_map, e2e) <= 1e-4
        check_map(out.rd_map, ref)
    else:
        K.check_case_map(c, out.rd_map, ref)
    want = K.oracle_dets(out.rd_map, c)
    np.testing.assert_array_equal(out.dets, want)
    np.testing.assert_array_equal(stage, want)
    assert len(want) >= 1
    if not c.compat_cfar and not q15:
        n, rel, frac = K.check_near_threshold(out.dets, ref, c, case)
        print(f"{case.id}: {n} decisions differ from the fp64 end to end, worst |cut-thr|/thr {rel:.3g}, "
              f"worst gap/margin {frac:.3g}")


def _run_integer(c, case, cube, capped=False, **over):
    """One handle: (process output, fmcw_cfar on its map, the range spectrum, a second process output).
    `capped`: under the case's grid caps, and then, with the caps at 0, the same four once more: the
    same bytes."""
    with make_core(c, case.nf, **over) as core:
        created = cap_grids(core, case) if capped else None
        out = core.process(cube)
        stage = run_cfar_stage(core, out.rd_map, cap=out.rd_map.size)
        spec = run_range_ct(core, cube, case.nf)
        assert core.info("range_kernel") == K.range_family(c)
        assert core.info("chunk") == (over.get("chunk_frames") or case.nf)
        again = core.process(cube)
        if created:
            uncap_grids(core, created)
            same_process(core.process(cube), out)
            same_bytes(run_cfar_stage(core, out.rd_map, cap=out.rd_map.size), stage)
            same_bytes(run_range_ct(core, cube, case.nf), spec)
    return out, stage, spec, again


def _same_output(a, b):
    np.testing.assert_array_equal(a.rd_map.view(np.uint32), b.rd_map.view(np.uint32))
    np.testing.assert_array_equal(a.dets, b.dets)
    assert (a.window_saturations, a.word_saturations) == (b.window_saturations, b.word_saturations)


@pytest.mark.parametrize("case", INTEGER, ids=lambda c: c.id)
def test_integer_path(gpu, case):
    """The integer datapath as a chain: i16 cube, the canceller on the spectrum's 16-bit words
    (FMCW_COMPAT_MTI or the Q15 window), the Hamming or the integer Doppler window after it, |X|
    with NCI or AMBM, CFAR.

    Map: per frame and per significant bin within 1e-4 of the oracle's Doppler stage in RTL
    arithmetic on the GPU's own range spectrum (a word rounds the same on both sides), and per
    frame within 1e-4 of the fp64 end to end.  AMBM: a bin may also be off by 2, because
    mx + floor(mn / 4) + floor(mn / 8) has two floor terms that each step by 1 when fp32 and fp64
    fall on different sides of an integer.  Detections, fused and stage: bit-exact against the oracle
    CFAR on the GPU's own map.  Status words 2 / 3: exactly the oracle's clips of the GPU's own
    spectrum plus the range window's clips of the cube -- 0 on the "int_clean" cubes, non-zero on
    "int_sat".  A second call on the same handle returns the same map, list and counts (the
    counters are re-armed per call).  One case runs again without FMCW_COMPAT_MTI (the Q15 window
    alone selects the words: identical bytes), one in two chunks against an unchunked handle."""
    c = case.cfg
    q15 = c.window == "q15_rtl"
    ambm = c.magnitude == "ambm"
    cube = K.make_cube(case)
    over = dict(chunk_frames=case.chunk_frames) if case.chunk_frames else {}
    out, stage, spec, again = _run_integer(c, case, cube, capped=True, **over)
    assert out.rd_map.shape == (case.nf, c.n_range, c.n_doppler)
    ref = K.int_map(c, spec)
    worst_frame = worst_bin = 0.0
    stepped = 0
    for f in range(case.nf):
        x = cube[f] if q15 else K.to_complex(cube[f], "i16")
        o = O.process(x, None, mti_mode=c.mti, q15_rtl=q15, mti_rtl=True, range_shift=c.range_shift)
        e2e = K.ambm_f64(o["rd"][0]) if ambm else o["mag"]
        got = out.rd_map[f].astype(np.float64)
        big = ref[f] >= 1e-3 * ref[f].max()
        err = np.abs(got[big] - ref[f][big])
        stepped += int((err > 1e-4 * ref[f][big]).sum())
        worst_bin = max(worst_bin, float(np.max((err - (2.0 if ambm else 0.0)) / ref[f][big])))
        worst_frame = max(worst_frame, rel_err(got, ref[f]), rel_err(got, e2e))
    print(f"{case.id}: worst frame rel err {worst_frame:.3g}, worst per-bin {worst_bin:.3g}"
          + (f", {stepped} bins beyond 1e-4 (within the 2 floor steps)" if ambm else ""))
    assert worst_frame <= 1e-4
    assert worst_bin <= 1e-4          # AMBM: |got - ref| <= 1e-4 ref + 2
    if not ambm:
        check_map(out.rd_map, ref)

    want = K.oracle_dets(out.rd_map, c)
    np.testing.assert_array_equal(out.dets, want)
    np.testing.assert_array_equal(stage, want)
    assert len(want) >= 1

    n = K.int_counts(c, cube, spec)
    print(f"{case.id}: clips {tuple(n)} (word, canceller, Doppler window, range window)")
    assert out.window_saturations == n.window_saturations
    assert out.word_saturations == n.word_saturations
    if case.recipe == "int_clean":
        assert out.window_saturations == 0 and out.word_saturations == 0 and not out.status_overflow
    else:
        assert n.word > 0 and n.canceller > 0 and out.status_overflow == q15
    _same_output(again, out)

    if case.id.endswith("compat-same"):
        assert q15 and c.compat_mti
        _same_output(_run_integer(dataclasses.replace(c, compat_mti=False), case, cube)[0], out)
    if case.chunk_frames:
        assert case.chunk_frames < case.nf
        _same_output(_run_integer(c, case, cube)[0], out)


@pytest.mark.parametrize("case", CFAR1D, ids=lambda c: c.id)
def test_cfar1d_stage_and_fused(gpu, case):
    """The same map through fmcw_cfar and, as a cube whose range-Doppler magnitude is that map,
    through the 1-D CFAR fused into K2: records bit-exact (indices, mag, threshold) against the
    oracle on the map each kernel saw."""
    c = case.cfg
    m = K.cfar1d_map(case)
    cube = K.cube_from_map(m)
    with make_core(c, case.nf) as core:
        created = cap_grids(core, case)
        stage, words = run_stage_words(core, m, cap=m.size)
        assert words[1] == 0
        out = core.process(cube)
        again = run_cfar_stage(core, out.rd_map, cap=m.size)
        if created:
            uncap_grids(core, created)
            stage0, words0 = run_stage_words(core, m, cap=m.size)
            same_bytes(stage0, stage)
            assert words0 == words
            same_process(core.process(cube), out)
    want, _, _ = K.cfar1d_oracle(m, c)
    np.testing.assert_array_equal(stage, want)
    # the fused kernel saw its own fp32 map: close to m, and decided exactly as the oracle on it
    assert rel_err(out.rd_map, m) <= 1e-4
    fused_want, _, _ = K.cfar1d_oracle(out.rd_map, c)
    np.testing.assert_array_equal(out.dets, fused_want)
    np.testing.assert_array_equal(again, fused_want)
    cells = lambda d: set(zip(d["frame"].tolist(), d["range"].tolist(), d["doppler"].tolist()))  # noqa: E731
    # the spikes survive the round trip: the fused list is not empty at the edges either
    assert {(0, 0, 0), (0, c.n_range - 1, c.n_doppler - 1)} <= cells(out.dets) & cells(stage)


@pytest.mark.parametrize("case", CFAR2D, ids=lambda c: c.id)
def test_cfar2d_stage(gpu, case):
    """fmcw_cfar with the 2-D CFAR on the case's crafted map, one launch of 3 frames at the case's
    strip length: records (indices, mag, threshold) bit-exact against cpu_backend.cfar (compat:
    fmcw_oracle.cfar_os2d_rtl), nothing dropped.  The rank-0 cases, where nearly every tested cell
    detects, run with det_capacity set, so their tiles overflow the slots into the shared region."""
    c = case.cfg
    m = K.cfar2d_map(case)
    over = dict(det_capacity=m.size) if K.cfar2d_dense(c) else {}
    with make_core(c, case.nf, **over) as core:
        if case.steps:
            core.set_param("cfar2d_steps", case.steps)
        created = cap_grids(core, case)
        got, words = run_stage_words(core, m, cap=m.size)
        assert words[1] == 0                               # nothing dropped
        if case.steps:
            per_frame = -(-c.n_range // K.cfar2d_TR(c.n_doppler))
            assert core.info("cfar2d_steps") == min(case.steps, per_frame)
        if created:
            uncap_grids(core, created)
            got0, words0 = run_stage_words(core, m, cap=m.size)
            same_bytes(got0, got)
            assert words0 == words
    if c.compat_cfar:
        want, _, _ = K.cfar2d_oracle(m, c)
    else:
        want = CB.cfar(K.cfar2d_clamped(m), K.oracle_cfar(c), threads=16, cap=m.size)
    print(f"{case.id}: {len(want)} detections")
    assert len(want) > 0
    np.testing.assert_array_equal(got, want)


def _enqueue_guarded(core, cube_dev, case, bufs):
    """One fmcw_enqueue into the sentinel-filled (map, records, status words) buffers: (map bytes as
    float32, records, status words), after checking the three tails."""
    c = case.cfg
    dmap, ddets, dn = bufs
    for b in bufs:
        b.fill()
    cap = ddets.nbytes // 16
    core.enqueue(cube_dev, case.nf, dmap.ptr, ddets.ptr, cap, dn.ptr)
    words = dn.get(np.uint32, (4,))          # a synchronous copy: behind the stream's work
    for b in bufs:
        b.check()
    assert words[0] <= cap and words[1] == 0, (words.tolist(), cap)
    return (dmap.get(np.float32, (case.nf, c.n_range, c.n_doppler)), ddets.get(DET_DTYPE, (int(words[0]),)),
            [int(w) for w in words])


@pytest.mark.parametrize("case", K.WHITE, ids=lambda c: c.id)
def test_whole_path_every_cell(gpu, case):
    """fmcw_enqueue on white full-scale noise, map, records and status words in guarded buffers filled
    with the sentinel: the tails intact, every map word written, every cell within 1e-4 of the rms of its
    range row of the fp64 oracle (kernel_matrix.check_every_cell: plus the format's bound on the fp16
    spectrum, plus AMBM's two floor steps), the records those of the oracle CFAR on the GPU's own map
    with nothing lost.  Under a capped grid, the same bytes once more with the caps at 0."""
    c = case.cfg
    cube, ref = K.reference(case)
    cells = case.nf * c.n_range * c.n_doppler
    over = dict(chunk_frames=case.chunk_frames) if case.chunk_frames else {}
    din = DeviceBuffer(cube.nbytes)
    bufs = (Guarded(cells * 4), Guarded(cells * 16), Guarded(16))
    try:
        din.upload(cube)
        with make_core(c, case.nf, **over) as core:
            created = cap_grids(core, case)
            got, dets, words = _enqueue_guarded(core, din, case, bufs)
            assert core.info("range_kernel") == K.range_family(c)
            if created:
                uncap_grids(core, created)
                got0, dets0, words0 = _enqueue_guarded(core, din, case, bufs)
                same_bytes(got0, got)
                same_bytes(dets0, dets)
                assert words0 == words
    finally:
        for b in bufs + (din,):
            b.free()
    assert_all_written(got, f"{case.id}: the map")
    K.check_every_cell(c, got, ref, case)
    np.testing.assert_array_equal(dets, K.oracle_dets(got, c))
    assert words[2] == 0 and words[3] == 0        # no integer window, no 16-bit words on this datapath
