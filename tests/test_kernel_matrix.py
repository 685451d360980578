"""CPU checks of the kernel test matrix (tests/kernel_matrix.py): the case table covers every
kernel variant the dispatch rules can reach, the rules agree with the kernels the built library
carries, and the cases' inputs are fair (a correct fp32 implementation passes them) and not
vacuous (the 1-D and 2-D CFAR maps have detections at every edge the kernels treat specially, and a
tie; the integer-path cubes clip nowhere or at every stage, as their recipe says), and the two CPU
references of the 2-D CFAR agree on every 2-D map."""
import dataclasses
import re
import subprocess

import numpy as np
import pytest

import cpu_backend as CB
import fmcw_oracle as O
import kernel_matrix as K
from test_abi import extract_code_objects

PROCESS = [c for c in K.CASES if c.group == "process"]
CFAR1D = [c for c in K.CASES if c.group == "cfar1d"]
CFAR2D = [c for c in K.CASES if c.group == "cfar2d"]
INTEGER = [c for c in PROCESS if c.recipe in ("int_clean", "int_sat")]
LOOPS = [c for c in K.CASES if c.grid]


def test_case_ids_unique_and_legal():
    ids = [c.id for c in K.CASES]
    assert len(ids) == len(set(ids))
    for c in K.CASES:
        assert K.legal(c.cfg), (c.id, K.illegal_reason(c.cfg))
        assert c.keys(), c.id


def test_cases_cover_every_reachable_variant():
    covered = set().union(*(c.keys() for c in K.CASES))
    missing = sorted(K.reachable() - covered)
    assert not missing, f"{len(missing)} variant keys no case runs:\n" + "\n".join(missing)
    stale = sorted(covered - K.reachable())
    assert not stale, f"cases claim keys the enumeration never reaches:\n" + "\n".join(stale)


def test_issue_variants_are_explicit_cases():
    """The variants the matrix was written for, by key."""
    covered = set().union(*(c.keys() for c in K.CASES))
    for key in ("cfar1d<64,8,2,multi-group>/stage", "cfar1d<64,8,2,multi-group>/fused-generic",
                "cfar1d<64,runtime>/window>halo/fused-generic", "cfar1d<256,runtime>/window>halo/stage",
                "cfar1d<32,runtime>/maximal/stage", "cfar1d<32,runtime>/maximal/fused-generic",
                "k_doppler<256,mti=2,F32,GEN>/pf=0", "k_doppler<1024,mti=3,F16,GEN>/pf=0",
                "k_doppler/nci<pf=16,F32>", "k_doppler/nci/odd-nrx",
                "k_doppler<64,mti=0,S48,FAST>/pf=16/per-point", "k_doppler<128,mti=0,S48,FAST>/pf=16/per-point",
                "k_doppler<1024,mti=0,S48S,FAST>/pf=0", "k_doppler<1024,mti=0,S48PS,FAST>/pf=0",
                "k_doppler/xcd-remap<NC=1024,B=6,T=4>", "k_doppler<1024,F32,GEN>/db", "k_doppler<32,F16,GEN>/ambm", "k_doppler<64,S48,GEN>/ambm",
                "k_range<512,LoadF16,false,0>/cw=0", "k_range<2048,LoadI16,false,0>/cw=0",
                "k_range<1024,LoadI16,false,4>/cw=1",
                # the integer datapath: the canceller on 16-bit words, the integer window after it
                "k_doppler<32,mti=2,F32,GEN>/words", "k_doppler<32,mti=3,F32,GEN>/words",
                "k_doppler<1024,mti=2,F32,GEN>/words", "k_doppler<1024,mti=3,F32,GEN>/words",
                "k_doppler<32,mti=2,F32,GEN>/words+q15d", "k_doppler<32,mti=3,F32,GEN>/words+q15d",
                "k_doppler<1024,mti=2,F32,GEN>/words+q15d", "k_doppler<1024,mti=3,F32,GEN>/words+q15d",
                # the 2-D CFAR: strips and the ring at the Doppler sizes that had one step or less
                "k_cfar2d<32,6,2,5,1>/step=partial", "k_cfar2d<32,0,0,0,0>/step=partial",
                "k_cfar2d<32,6,2,5,1>/strip=up", "k_cfar2d<32,0,0,0,0>/strip=down",
                "k_cfar2d<64,6,2,5,1>/strip=short-last", "k_cfar2d<64,0,0,0,0>/strip=up",
                "k_cfar2d<256,0,0,0,0>/strip=one-step", "k_cfar2d<512,6,2,5,1>/strip=down",
                "k_cfar2d_lv<1024,5,1,false>/strip=up", "k_cfar2d_lv<1024,5,1,true>/strip=short-last",
                # the generic kernel's runtime geometry
                "k_cfar2d<64,0,0,0,0>/window>halo", "k_cfar2d<1024,0,0,0,0>/window>halo",
                "k_cfar2d<32,0,0,0,0>/maximal", "k_cfar2d<128,0,0,0,0>/hr=0", "k_cfar2d<32,0,0,0,0>/hd=0",
                "k_cfar2d<512,0,0,0,0>/hr>=TR", "k_cfar2d<1024,0,0,0,0>/hr>=TR",
                # parameters
                "k_cfar2d<128,0,0,0,0>/compat", "k_cfar2d<256,6,2,5,1>/compat", "k_cfar2d_decide<64>/compat",
                "k_cfar2d<64,0,0,0,0>/override", "k_cfar2d_lv<1024,5,1,true>/override",
                "k_cfar2d_decide<32>/override", "k_cfar2d_decide<32>/n_ref<=64", "k_cfar2d_decide<512>/n_ref=pow2",
                "k_cfar2d_decide<512>/n_ref=div", "k_cfar2d<32,6,2,5,1>/rank=0", "k_cfar2d_decide<1024>/rank=0",
                "k_cfar2d<1024,0,0,0,0>/rank=n_ref-1", "k_cfar2d_decide<128>/rank=n_ref-1"):
        assert key in covered, key
    # every Doppler size: the two windows at strips of 1, 3, 5 and the cost model's, every legal
    # window, compat, both rank ends, an override and both extra scale sets
    for nc in K.N_DOPPLER:
        mine = [c for c in CFAR2D if c.cfg.n_doppler == nc and c.cfg.n_range == K.cfar2d_shape(nc)]
        for w in K.CFAR2D_SETS[:2]:
            got = {(c.steps, c.cfg.compat_cfar, c.cfg.cfar2d_rank_pct, c.cfg.cfar2d_override, c.cfg.cfar2d_scales)
                   for c in mine if c.cfg.cfar2d == w}
            assert {(s, False, 75, 0, (2, 4, 6)) for s in (0, 1, 3, 5)} <= got
            assert {(3, True, 75, 0, (2, 4, 6)), (3, False, 0, 0, (2, 4, 6)), (3, False, 100, 0, (2, 4, 6)),
                    (3, False, 75, 3, (2, 4, 6)), (3, False, 75, 0, (2, 2, 2)), (3, False, 75, 0, (1, 3, 5))} <= got
        legal = {w for w in K.CFAR2D_SETS if K.legal(K.Cfg(n_doppler=nc, cfar="os2d", cfar2d=w))}
        assert legal == {c.cfg.cfar2d for c in mine}
    assert all(c.nf == 3 and c.cfg.n_range * c.cfg.n_doppler <= 1 << 16 for c in CFAR2D)
    geoms = {(c.cfg.n_range, c.cfg.n_doppler) for c in PROCESS if c.cfg.spectrum == "s48"}
    assert {(64, 64), (128, 64), (256, 64), (512, 64), (128, 128), (1024, 1024), (2048, 1024)} <= geoms
    assert any(c.cfg.n_range == 1024 and c.cfg.n_doppler == 256 and c.cfg.n_rx == 2 for c in PROCESS)
    # the integer datapath: at every Doppler size and canceller, the word canceller under the
    # Hamming and the Q15 window on a cube that clips nowhere and on one that clips, and the chain
    for nc in K.N_DOPPLER:
        for m in (2, 3):
            got = {(c.cfg.window, c.cfg.compat_mti, c.recipe, c.cfg.magnitude, c.cfg.compat_cfar) for c in INTEGER
                   if c.cfg.n_doppler == nc and c.cfg.mti == m and c.cfg.n_range == 64}
            assert {("hamming", True, "int_clean", "abs", False), ("hamming", True, "int_sat", "abs", False),
                    ("q15_rtl", False, "int_clean", "abs", False), ("q15_rtl", False, "int_sat", "abs", False),
                    ("q15_rtl", True, "int_clean", "ambm", True)} <= got
    assert any(c.chunk_frames and c.nf > c.chunk_frames and c.recipe == "int_sat" for c in INTEGER)
    # the persistent loops: one key per kernel family and addressing mode, both XCD forms, K3 at the
    # smallest and the largest Doppler size
    for key in ("k_range<64,LoadF32,false,0>/cw=0/loop", "k_range<2048,LoadI16,true,0>/cw=0/loop",
                "k_range<512,LoadF16,false,1>/cw=1/loop", "k_range<256,LoadI16,false,1>/cw=0/loop",
                "k_range<128,LoadF32,false,2>/cw=1/loop", "k_range<1024,LoadI16,false,4>/cw=1/loop",
                "k_range<2048,LoadF16,false,5>/cw=1/loop", "k_range_sq<4096,LoadI16,16,1,3,0>/cw=1/loop",
                "k_range_sq<4096,LoadF32,16,1,3,5>/cw=1/loop", "k_range_px<LoadF16,4,4,0>/cw=0/loop",
                "k_range_px<LoadI16,4,6,5>/cw=1/loop",
                "k_doppler<32,mti=0,F32,FAST>/pf=16/per-point/loop", "k_doppler<32,mti=0,F16,GEN>/pf=16/uniform/loop",
                "k_doppler<256,mti=0,F32,FAST>/pf=16/uniform/loop", "k_doppler<512,mti=0,F32,GEN>/pf=8/uniform/loop",
                "k_doppler<1024,mti=0,F32,FAST>/pf=0/loop", "k_doppler<64,mti=2,F32,GEN>/pf=0/loop",
                "k_doppler<1024,mti=3,F16,GEN>/pf=0/loop", "k_doppler<64,mti=0,S48,FAST>/pf=16/per-point/loop",
                "k_doppler<128,mti=0,S48,GEN>/pf=16/uniform/loop", "k_doppler<256,mti=0,S48S,FAST>/pf=16/strided/loop",
                "k_doppler<512,mti=0,S48PS,GEN>/pf=8/strided/loop", "k_doppler<1024,mti=0,S48S,FAST>/pf=0/loop",
                "k_doppler/nci<pf=16,F32>/loop", "k_doppler/nci<pf=8,F16>/loop", "k_doppler/nci<pf=0,F32>/loop",
                "k_doppler/nci<pf=16,S48>/loop", "k_doppler/nci<pf=16,S48S>/loop", "k_doppler/nci<pf=0,S48PS>/loop",
                "k_doppler/xcd-remap<NC=1024,B=8,T=2>/loop", "k_doppler/xcd-remap<NC=1024,B=6,T=4>/loop",
                "k_doppler/xcd-remap<NC=1024,B=6,T=2>/loop", "k_doppler/xcd-remap<NC=512,B=6,T=2>/loop",
                "k_doppler<32>/tile-order=frame-minor/loop", "k_doppler<32>/tile-order=grouped/loop",
                "k_doppler<1024>/tile-order=grouped/loop",
                "k_cfar1d<32>/loop", "k_cfar1d<1024>/loop",
                "k_cfar2d<32,0,0,0,0>/loop", "k_cfar2d<32,6,2,5,1>/loop", "k_cfar2d<1024,0,0,0,0>/loop",
                "k_cfar2d_lv<1024,5,1,false>/loop", "k_cfar2d_lv<1024,5,1,true>/loop",
                "k_cfar2d_decide<32>/loop", "k_cfar2d_decide<1024>/loop", "k_cfar2d_emit<32>/loop",
                "k_cfar2d_emit<1024>/loop"):
        assert key in covered, key
    # every loop case is a case of the table above with a grid of 1, 2, 3 or 16 (and more frames);
    # nothing is larger than 2048 x 1024 x 1 frame unless its base case already was
    by_id = {c.id: c for c in K.CASES}
    for c in LOOPS:
        b = by_id[K.LOOP_BASE[c.id]]
        assert not b.grid and c.grid in K.LOOP_GRIDS and c.cfg == b.cfg and (c.group, c.recipe, c.steps) == (b.group, b.recipe, b.steps)
        assert c.nf >= b.nf and (c.seed >= 9000 or c.recipe == "int_clean" and c.seed == b.seed) and c.id.endswith(f"-loop-g{c.grid}")
        cells = lambda x: x.cfg.n_range * x.cfg.n_doppler * x.cfg.n_rx * x.nf  # noqa: E731
        assert cells(c) <= max(K.MAX_CELLS, cells(b)), c.id
    sat = [c for c in LOOPS if c.recipe == "int_sat"]
    assert any(c.cfg.window == "q15_rtl" for c in sat) and any(c.cfg.compat_mti and c.cfg.window == "hamming" for c in sat)
    # the chunked one: every launch of the call loops, and the second starts beyond frame 0
    assert any(c.chunk_frames and K.launch_frames(c.nf, c.chunk_frames) == [c.chunk_frames] * 2 for c in sat)
    # NCI under a capped grid: an even and an odd n_rx on kernels with and without a prefetch
    nci = {(K.k2_prefetch(c.cfg.n_doppler, c.cfg.mti) > 0, c.cfg.n_rx % 2) for c in LOOPS
           if c.group == "process" and c.cfg.n_rx > 1 and "k2" in c.loops()}
    assert nci == {(True, 0), (True, 1), (False, 0), (False, 1)}
    for nc in K.N_DOPPLER:          # K3a: the generic, the level-screen / lv and the compat kernel, strips of 3
        got = {(c.cfg.cfar2d, c.cfg.compat_cfar) for c in LOOPS if c.group == "cfar2d" and c.cfg.n_doppler == nc
               and c.steps == 3 and "k3a" in c.loops()}
        assert {(K.CFAR2D_SETS[0], False), (K.CFAR2D_SETS[1], False), (K.CFAR2D_SETS[0], True)} <= got


def _stride(units, grid):
    """The loop as the kernels write it: for (g = blockIdx.x; g < units; g += gridDim.x), under the
    launch sites' grid of min(units, cap)."""
    n = min(units, grid)
    return [[g for g in range(b, units, n)] for b in range(n)]


@pytest.mark.parametrize("case", LOOPS, ids=lambda c: c.id)
def test_loop_case_runs_its_loops(case):
    """Every "/loop" key a case claims, recomputed here from the unit counts of the launch sites and
    the loops as the kernels write them: the busiest workgroup runs at least 3 iterations in every
    launch of the call, and its last has no next unit.  K2 per wave (tile = bid WPB + wave, step grid
    WPB, doppler_kernel.hpp k_doppler tile loop), with the XCD remap a permutation that is not the identity; K3a with a down
    strip right after an up strip and an up strip right after a down strip in one workgroup (strips of
    one step: two frames in a row); K3c per wave of the 4 grid waves.  A case with a grid claims at
    least one such key."""
    c, G = case.cfg, case.grid
    claimed = {k[:-5] for k in case.keys() if k.endswith("/loop")}
    assert claimed, "a capped grid that loops nowhere"
    assert all(k in case.keys() for k in claimed)
    kernels = {K.loop_kernel(k) for k in claimed}
    T = 16 if c.n_range <= 128 else 8 if c.n_range <= 512 else 4 if c.n_range == 1024 else 2    # range_kernels.hpp RangeGeom<N>::T
    wr = 64 // (c.n_doppler // 16)                                                                # cfar1d.hpp DopplerGeom::WR
    per_launch = K.launch_frames(case.nf, case.chunk_frames) if case.group in ("process", "cfar1d") else [case.nf]
    assert sum(per_launch) == case.nf and (not case.chunk_frames or max(per_launch) == case.chunk_frames < case.nf)
    if "k1" in kernels:
        for n in per_launch:
            walks = _stride(n * c.n_rx * c.n_doppler // T, G)                                   # launch.hip launch_range n_groups
            assert max(map(len, walks)) >= 3
            assert all(w[-1] + len(walks) >= n * c.n_rx * c.n_doppler // T for w in walks)
    if kernels & {"k2", "xcd", "cfar1d"}:
        for n in per_launch:
            n_tiles = n * (c.n_range // wr)                                                      # launch.hip tile_grid
            grid = min(-(-n_tiles // 4), G)                                                      # tile_grid: min(ceil(n_tiles / wpb), grid.doppler)
            per_wave = []
            for b in range(grid):
                remap = "xcd" in kernels and grid % 8 == 0
                bid = (b & 7) * (grid >> 3) + (b >> 3) if remap else b                           # doppler_kernel.hpp xcd_block_id
                per_wave += [list(range(bid * 4 + wv, n_tiles, grid * 4)) for wv in range(4)]
            assert sorted(t for w in per_wave for t in w) == list(range(n_tiles))               # every tile once
            assert max(map(len, per_wave)) >= 3
            assert all(w[-1] + grid * 4 >= n_tiles for w in per_wave if w)
            if "xcd" in kernels:     # a grid of 8 is a multiple of 8 too, but maps every block to itself
                assert grid % 8 == 0
                assert [(b & 7) * (grid >> 3) + (b >> 3) for b in range(grid)] != list(range(grid))
    if kernels & {"k3a", "k3b", "k3c"}:
        assert case.group == "cfar2d" and case.steps
        tr = 4 * wr                                                                              # cfar2d.hpp Cfar2DGeom::TR
        tpf = -(-c.n_range // tr)                                                                # launch.hip launch_cfar tpf
        steps = min(case.steps, tpf)
        spf = -(-tpf // steps)
        walks = _stride(case.nf * spf, G)                                                        # launch.hip launch_cfar n_strips, grid
        if "k3a" in kernels:
            assert max(map(len, walks)) >= 3
            ok = False
            for w in walks:
                seq = []
                for g in w:
                    f, i = g % case.nf, g // case.nf                                             # cfar2d.hpp k_cfar2d strip loop
                    n_steps = min(i * steps + steps, tpf) - i * steps
                    seq.append((f, None if n_steps == 1 else bool(i & 1)))                       # k_cfar2d `up`, `first` / `last`
                pairs = list(zip(seq, seq[1:]))
                if all(d is None for _, d in seq):
                    ok |= any(a[0] != b[0] for a, b in pairs)
                else:
                    ok |= (any(a[1] is True and b[1] is False for a, b in pairs)
                           and any(a[1] is False and b[1] is True for a, b in pairs))
            assert ok
        if "k3c" in kernels:
            assert -(-case.nf * (c.n_range // wr) // (4 * G)) >= 3


@pytest.mark.parametrize("case", [c for c in LOOPS if c.group == "cfar2d"], ids=lambda c: c.id)
def test_cfar2d_loop_case_has_candidates(case):
    """K3b strides over the candidates, 4 waves per workgroup and one candidate per wave at a time
    (cfar2d.hpp cfar2d_decide_run); their number depends on the data, and every detection was a candidate.
    The oracle's detections on the case's map, all in one launch (3 frames), are at least 3 per wave
    of the capped grid."""
    dets, _, _ = _oracle2d(case)
    assert case.nf == 3
    assert len(dets) >= 3 * 4 * case.grid, len(dets)


def _kernel_symbols(tmp_path):
    _, cos = extract_code_objects(tmp_path)
    if not cos:
        pytest.skip("this llvm-objdump cannot extract offload bundles")
    names = set()
    for co in cos:
        out = subprocess.run(["readelf", "-sW", str(co)], capture_output=True, text=True, check=True).stdout
        mangled = [ln.split()[7] for ln in out.splitlines() if len(ln.split()) >= 8 and ln.split()[3] == "FUNC"]
        dem = subprocess.run(["c++filt"], input="\n".join(mangled), capture_output=True, text=True, check=True).stdout
        for ln in dem.splitlines():
            m = re.match(r"(?:void )?fmcw::(k_\w+(?:<.*>)?)\(", ln)
            if m:
                names.add(m.group(1))
    return names


def test_mirror_matches_the_library(lib_built, tmp_path):
    """Every kernel a reachable key names is in the gfx950 code objects, and every K1 / K2 / CFAR
    kernel there is either reachable or listed in UNREACHABLE with its reason (symbol names only)."""
    have = _kernel_symbols(tmp_path)
    want = {s for s in K.reachable_with_symbols().values() if s}
    assert not sorted(want - have), f"the mirror names kernels the library lacks: {sorted(want - have)}"
    table = {s for s in have if re.match(r"k_(range|doppler|cfar1d|cfar2d)", s)}
    assert len(table) > 200
    unknown = sorted(table - want - set(K.UNREACHABLE))
    assert not unknown, "kernels neither reachable nor in UNREACHABLE:\n" + "\n".join(unknown)
    stale = sorted(s for s in K.UNREACHABLE if s not in have or s in want)
    assert not stale, f"UNREACHABLE entries that are reachable or gone: {stale}"
    assert all(K.UNREACHABLE.values())


def _fp32_runnable(case):
    c = case.cfg
    return (c.mti == 0 and c.magnitude == "abs" and c.map_kind == "linear" and c.window == "hamming"
            and not c.compat_cfar and c.range_shift == 0)


@pytest.mark.parametrize("case", [c for c in PROCESS if _fp32_runnable(c)], ids=lambda c: c.id)
def test_case_is_fair_to_fp32(case):
    """The C fp32 restatement of the pipeline, on the case's input, stays inside the bounds the
    GPU test applies: the inputs themselves do not push a correct fp32 implementation out."""
    c = case.cfg
    cube, ref = K.reference(case)
    x = K.to_complex(cube, c.in_dtype).astype(np.complex64)
    got, dets, n = CB.process(x, K.oracle_cfar(c), threads=4)
    assert n == len(dets)
    # the restatement keeps an fp32 spectrum: it is held to the fp32 rule whatever the case's spectrum
    fp32 = dataclasses.replace(c, spectrum="f32")
    K.check_case_map(fp32, got, ref)
    K.check_near_threshold(dets, ref, fp32)


def _fp16(z):
    return z.real.astype(np.float16).astype(np.float64) + 1j * z.imag.astype(np.float16).astype(np.float64)


@pytest.mark.parametrize("case", [c for c in PROCESS if c.cfg.spectrum == "f16" and c.cfg.magnitude == "abs"],
                         ids=lambda c: c.id)
def test_case_is_fair_to_the_fp16_spectrum(case):
    """The fp16 spectrum's rule is 2e-3 of the frame's peak.  The format alone, applied in fp64 to the
    oracle's range spectrum (half2(X / N_range), fmcw.h FMCW_SPEC_F16), must leave the case's map
    within 1.9e-3 (the rest is the fp32 arithmetic's 1e-4): with MTI on, a target near zero Doppler
    is cancelled, the frame's peak falls to the clutter's level, and no implementation of the format
    meets the rule on that cube (kernel_matrix.LOOP_SEED_MOVED)."""
    c = case.cfg
    cube, ref = K.reference(case)
    for f in range(case.nf):
        spec = O.range_ct(K.to_complex(cube[f], c.in_dtype)) * 2.0 ** -c.range_shift
        rd = O.doppler_stage(_fp16(spec / c.n_range) * c.n_range, mti_mode=c.mti)
        e = np.abs(O.magnitude(rd, rx_axis=0) - ref[f]).max() / ref[f].max()
        assert e <= 1.9e-3, f"frame {f}: the format alone moves the map by {e:.3g} of its peak"


@pytest.mark.parametrize("case", [c for c in LOOPS if c.group == "process" and c.cfg.mti == 3 and c.cfg.window == "hamming"
                                  and c.cfg.spectrum == "f32" and c not in INTEGER], ids=lambda c: c.id)
def test_mti_case_keeps_every_frames_target(case):
    """The 3-pulse canceller removes a target near zero Doppler, and its frame's peak falls to the
    clutter's level, where K1's fp32 rounding of the uncancelled spectrum shows beyond the per-bin
    1e-4 (seen at 1 / 70 of the other frames' peak and below; kernel_matrix.LOOP_SEED_MOVED).  Every
    frame's peak in the fp64 oracle's map is within a factor of 32 of the case's largest."""
    _, ref = K.reference(case)
    peaks = [float(ref[f].max()) for f in range(case.nf)]
    assert min(peaks) >= max(peaks) / 32, peaks


@pytest.mark.parametrize("case", CFAR1D, ids=lambda c: c.id)
def test_cfar1d_case_is_not_vacuous(case):
    """The oracle's detections on the case's map touch Doppler cells 0 and NC - 1, both ends of a
    lane's 16-cell block, the first and the last range row; and some cell ties with its threshold
    (cut == threshold: not a detection)."""
    c = case.cfg
    m = K.cfar1d_map(case)
    assert np.array_equal(m, np.floor(m)) and m.min() >= 0
    dets, mask, thr = K.cfar1d_oracle(m, c)
    d, r = dets["doppler"].astype(int), dets["range"].astype(int)
    assert (d == 0).any() and (d == c.n_doppler - 1).any()
    assert (d % 16 == 0).any() and (d % 16 == 15).any()
    assert (r == 0).any() and (r == c.n_range - 1).any()
    cut = np.minimum(np.floor(m), 131071.0) if c.compat_cfar else m
    tie = (cut == thr) & (m > 0)
    assert tie.any() and not mask[tie].any()
    assert 0 < len(dets) < m.size
    # the two cells at the edge of the group screen (cfar1d_map rows 30, 33): exactly 4 / ref
    # references reach cut / alpha, and the oracle detects iff that count is below n_ref - rank
    ref, guard, rank, alpha = c.cfar1d
    dc = c.n_doppler // 2 + 3
    offs = [-(guard + 1 + j) for j in range(ref)] + [guard + 1 + j for j in range(ref)]
    for row, n_high in ((30, 4), (33, ref)):
        refs = np.array([m[0, row, (dc + o) % c.n_doppler] for o in offs], np.float32)
        assert int((np.float32(alpha) * refs >= m[0, row, dc]).sum()) == n_high
        assert bool(mask[0, row, dc]) == (n_high < 2 * ref - rank)


def _components(z):
    return np.stack([z.real, z.imag])


@pytest.mark.parametrize("case", INTEGER, ids=lambda c: c.id)
def test_integer_case_is_not_vacuous(case):
    """The fp64 oracle alone on an integer-path case.  "int_clean": nothing clips at any of the four
    places, at the smallest such range_shift, and the largest word after the canceller is at least
    2^13 (the word range is used).  "int_sat": the spectrum words, the canceller and, with the Q15
    window, both windows clip; the counts differ between the frames and between the rx channels; the
    3-pulse canceller has a sample beyond 2 x 32768, which only its gain of 4 reaches.  Every case:
    at least one detection under its CFAR.  "int_clean": every frame's peak is at least 2^11 x
    n_doppler, a quarter of what a full-scale word gives (8192 x 0.54 x n_doppler x the canceller's
    gain of 2), so no frame is compared at the level of single word roundings; at 2^16 and above
    the two floor steps of AMBM are below a third of the frame-level 1e-4.  The chain (AMBM, integer
    CFAR): the noise floor lies inside the 17-bit CFAR word."""
    c = case.cfg
    q15 = c.window == "q15_rtl"
    cube = K.make_cube(case)
    assert cube.dtype == np.int16 and cube.shape == (case.nf, c.n_rx, c.n_doppler, c.n_range, 2)
    assert c.in_dtype == "i16" and c.mti in (2, 3) and (c.compat_mti or q15)
    spec = K.int_spectrum(case, cube)
    n = K.int_counts(c, cube, spec)
    words = O.spectrum_words(spec)
    if case.recipe == "int_clean":
        assert n == O.WordClips(0, 0, 0, 0)
        assert np.abs(_components(O.mti_spectrum_rtl(spec, c.mti))).max() >= 2 ** 13
        assert sum(K.int_counts(c, cube, 2.0 * spec)) > 0          # range_shift - 1 clips
    else:
        assert n.word > 0 and n.canceller > 0
        assert (n.doppler_window > 0 and n.range_window > 0) if q15 else (n.doppler_window == n.range_window == 0)
        per_frame = [tuple(K.int_counts(c, cube[f:f + 1], spec[f:f + 1])) for f in range(case.nf)]
        per_rx = [tuple(K.int_counts(c, cube[:, r:r + 1], spec[:, r:r + 1])) for r in range(c.n_rx)]
        assert len(set(per_frame)) == case.nf and len(set(per_rx)) == c.n_rx == 2
        assert tuple(map(sum, zip(*per_frame))) == tuple(n) == tuple(map(sum, zip(*per_rx)))
        w = _components(words)
        if c.mti == 3:
            assert (np.abs(w[..., 2:] - 2 * w[..., 1:-1] + w[..., :-2]) > 2 * 32768).any()
        # consecutive words of the target alternate in sign: the 2-pulse difference leaves int16 too
        assert (np.abs(w[..., 1:] - w[..., :-1]) > 32768).any()
    m = K.int_map(c, spec)
    assert len(K.oracle_dets(m.astype(np.float32), c)) >= 1
    if case.recipe == "int_clean":
        # every frame's target survives the canceller (kernel_matrix.INT_SEED_MOVED)
        assert min(m[f].max() for f in range(case.nf)) >= 2 ** 11 * c.n_doppler >= 2 ** 16
    if c.magnitude == "ambm":
        assert c.compat_cfar and c.n_rx == 1
        assert 8 <= np.median(m) <= 2 ** 13
    # the map from the spectrum is the end-to-end oracle's
    x0 = cube[0] if q15 else K.to_complex(cube[0], "i16")
    e2e = O.process(x0, None, mti_mode=c.mti, q15_rtl=q15, mti_rtl=True, range_shift=c.range_shift)
    np.testing.assert_array_equal(K.ambm_f64(e2e["rd"][0]) if c.magnitude == "ambm" else e2e["mag"], m[0])


_ORACLE_DETS = {}       # case id -> the NumPy oracle's records, computed once for both tests below


def _oracle2d(case):
    if case.id not in _ORACLE_DETS:
        dets, mask, thr = K.cfar2d_oracle(K.cfar2d_map(case), case.cfg)
        _ORACLE_DETS[case.id] = dets
        return dets, mask, thr
    return _ORACLE_DETS[case.id], None, None


def _cells(d):
    return d["frame"].astype(int), d["range"].astype(int), d["doppler"].astype(int)


@pytest.mark.parametrize("case", CFAR2D, ids=lambda c: c.id)
def test_cfar2d_case_is_not_vacuous(case):
    """The oracle's detections on the case's map (kernel_matrix.cfar2d_layout) touch every edge K3
    treats specially, reach every scale the bracket can choose, and leave a tie undetected.

    Doppler cells 0, 15, 16 and NC - 1; the first and last tested rows and none outside them; both
    rows at every step boundary; with no override and three different scales, each scale the bracket
    can reach chosen for a detection and for a tested cell that is none (frame 0, where the hand-made
    windows lie; rank 0 cannot reach scale_max -- the smallest reference is never above the mean --
    and rank n_ref - 1 cannot reach scale_min); the +0 and denormal cells; for rank 0 a step with more
    than kCoopRound detections and a wave tile beyond its slot."""
    c = case.cfg
    ns, nc, tr = c.n_range, c.n_doppler, K.cfar2d_TR(c.n_doppler)
    hr, _, _, _, n_ref, rank = K.cfar2d_geom(c)
    m, marks = K.cfar2d_layout(case)
    assert m.shape == (3, ns, nc) and m.dtype == np.float32
    if c.compat_cfar:
        assert np.array_equal(m, np.floor(m)) and m.max() <= 60000
    else:
        assert m.max() == np.float32(1e30)
    assert (m < 0).any() and np.signbit(m[m == 0]).any()
    _ORACLE_DETS.pop(case.id, None)
    dets, mask, thr = _oracle2d(case)
    f, r, d = _cells(dets)
    assert 0 < len(dets)
    assert (d == 0).any() and (d == nc - 1).any()
    assert (d % 16 == 0).any() and (d % 16 == 15).any() and (d == 15).any() and (d == 16).any()
    assert (r == hr).any() and (r == ns - hr - 1).any()
    assert r.min() >= hr and r.max() < ns - hr
    tested, untested = K.cfar2d_spike_rows(case)
    for row in tested:          # the first and last tested rows, both rows at every step boundary
        assert (r == row).any(), row
    for k in range(1, -(-ns // tr)):
        assert {k * tr - 1, k * tr} <= set(tested) | set(untested)
    if case.steps:              # every strip boundary of the case is a step boundary
        for i, _ in K.cfar2d_strips(ns, nc, case.steps)[1:]:
            assert i * min(case.steps, -(-ns // tr)) * tr in set(tested) | set(untested)
    for row in untested:        # spikes in rows whose range extent leaves the map: in no list
        assert (m[:, row] >= 50000).any() and not (r == row).any()
    # the tie and the hand-made windows
    assert m[marks["tie"]] == thr[marks["tie"]] > 0 and not mask[marks["tie"]]
    for name, at in marks.items():
        assert bool(mask[at]) == name.endswith("_det"), name
        if name.endswith("_tie"):
            assert m[at] == thr[at], name
    assert m[marks["zero_det"]] > 0 and thr[marks["zero_det"]] == 0
    z = marks["zero_cut0"]
    assert m[z] == 0 and not np.signbit(m[z]) and thr[z] == 0
    if not c.compat_cfar:
        assert 0 < m[marks["denorm_det"]] < np.finfo(np.float32).tiny
    # the scale of every tested cell of frame 0: threshold / ranked, the ranked value being the
    # oracle's threshold under a scale override of 1
    scales = K.cfar2d_scales_reachable(c)
    if not c.cfar2d_override and len(set(c.cfar2d_scales)) == 3:
        _, _, ranked = K.cfar2d_oracle(m, dataclasses.replace(c, cfar2d_override=1), frames=(0,))
        ranked, t0, det0 = ranked[0, hr:ns - hr], thr[0, hr:ns - hr], mask[0, hr:ns - hr]
        for s in scales:
            chosen = (ranked > 0) & (t0 == np.float32(s) * ranked)
            assert (chosen & det0).any() and (chosen & ~det0).any(), s
        assert ((ranked == 0) | np.any([t0 == np.float32(s) * ranked for s in scales], axis=0)).all()
    else:
        assert {"max_det", "min_det"}.isdisjoint(marks) or len(set(c.cfar2d_scales)) < 3
    if K.cfar2d_dense(c):
        # a second coop_rounds round (more than kCoopRound survivors in a step of 4096 cells: L = 1)
        # and, with det_capacity set, a wave tile (1024 cells) beyond its slot: the overflow region
        coop, slot_floor, slot_div = K.cfar2d_source_constants()
        per_step = np.bincount(f * ns // tr + r // tr)
        per_tile = np.bincount((f * ns + r) // (1024 // nc))
        assert per_step.max() > coop
        assert per_tile.max() > max(slot_floor, 1024 // slot_div)
        assert len(dets) > m.size // 2


@pytest.mark.parametrize("case", [c for c in CFAR2D if not c.cfg.compat_cfar], ids=lambda c: c.id)
def test_cfar2d_references_agree(case):
    """cpu_backend.cfar (the C oracle the GPU test compares against) and fmcw_oracle.cfar_os2d return
    identical records on the case's map."""
    m = K.cfar2d_map(case)
    want, _, _ = _oracle2d(case)
    got = CB.cfar(K.cfar2d_clamped(m), K.oracle_cfar(case.cfg), threads=4, cap=m.size)
    np.testing.assert_array_equal(got, want)


# ---- the white scene (kernel_matrix.WHITE): every cell of the K1 -> K2 map is checked ---------------
WHITE_F16 = [c for c in K.WHITE if c.cfg.spectrum == "f16"]


def test_white_cases_cover_every_k1_k2_key():
    """Every K1 / K2 key of reachable() that loopable() accepts, its "/loop" twin, and the AMBM branch has a
    white twin -- but for the keys no admissible whole-path case of CASES runs (the Q15 window and the
    integer datapath are left out): K1 launched without the fused Doppler weight ("/cw=0": fmcw_range_ct,
    the Q15 window, the integer cases; test_range_stage runs those on white noise per bin already) and the
    two loop twins of the generic fp32 K2 at NC 32, which only the Q15 cases run under a capped grid."""
    wanted = {k for k in K.reachable() if K.white_wanted(k)}
    covered = set().union(*(c.keys() for c in K.WHITE))
    left_out = {k for k in wanted if "/cw=0" in k and k.startswith("k_range")} \
        | {"k_doppler<32,mti=0,F32,GEN>/pf=16/per-point/loop", "k_doppler<32,mti=0,F32,GEN>/pf=16/uniform/loop"}
    missing = sorted(wanted - covered - left_out)
    assert not missing, f"{len(missing)} K1 / K2 keys without a white twin:\n" + "\n".join(missing)
    # what is left out by rule and has a white twin all the same (K1 without the weight under MTI)
    print(f"{len(wanted)} keys, {len(covered & wanted)} with a white twin, {len(left_out - covered)} left out")
    for sym in {s for k, s in K.reachable_with_symbols().items() if s and s.startswith("k_doppler")}:
        assert any(sym == s for c in K.WHITE for _, s in c.selected()), sym      # every K2 kernel
    k1 = {s for k, s in K.reachable_with_symbols().items() if s and s.startswith("k_range") and ", true, " not in s}
    assert k1 == {s for c in K.WHITE for _, s in c.selected() if s and s.startswith("k_range")}   # every K1 kernel but Q15's


def test_white_cases_are_twins():
    ids = [c.id for c in K.WHITE]
    assert len(ids) == len(set(ids)) and not set(ids) & {c.id for c in K.CASES}
    by_id = {c.id: c for c in K.CASES}
    assert [c.seed for c in K.WHITE] == list(range(K.WHITE_SEED, K.WHITE_SEED + len(K.WHITE)))
    for c in K.WHITE:
        b = by_id[K.WHITE_BASE[c.id]]
        assert c.id == b.id + "-white" and c.recipe == "uniform" and c.group == "process" and K.legal(c.cfg)
        assert c.cfg == dataclasses.replace(b.cfg, map_kind="linear") and c.cfg.window == "hamming"
        assert (c.nf, c.grid, c.chunk_frames, c.steps) == (b.nf, b.grid, b.chunk_frames, b.steps)
        assert b.recipe in ("random_target", "two_targets")
        assert c.cfg.n_range * c.cfg.n_doppler * c.nf <= K.MAX_CELLS, c.id
    assert sum(c.cfg.map_kind == "db" for c in by_id.values()) and not any("-db-" in i for i in ids)


@pytest.mark.parametrize("case", K.WHITE, ids=lambda c: c.id)
def test_white_case_checks_every_cell(case):
    """On the fp64 oracle alone: zeros, the reference rolled by one range row or one Doppler bin, and the
    previous frame's map pass the every-cell rule in at most 2 % of the cells (25 % under the fp16
    spectrum's rule, which carries the format's worst-case bound)."""
    c = case.cfg
    _, ref = K.reference(case)
    sh = K.unchecked_shares_map(ref, K.every_cell_bound(c, ref, case))
    print(f"{case.id}: unchecked shares " + ", ".join(f"{k} {v:.4f}" for k, v in sh.items()))
    cap = K.WHITE_CAP_F16 if c.spectrum == "f16" else K.WHITE_CAP
    assert sh["frame"] == 1.0 if case.nf == 1 else sh["frame"] <= cap
    assert max(sh["zero"], sh["row"], sh["bin"]) <= cap, sh


@pytest.mark.parametrize("case_id", ["process-k2-256-f32-fast-config2-nrx2", "process-k2-1024-s48-pair-fast-nrx2"])
def test_tone_scene_leaves_most_cells_unchecked(case_id):
    """Why the white scene exists: on the tone scene of these two cases (1024 x 256, the bench shape, and
    2048 x 1024) a map of zeros, or the reference one range row or one Doppler bin off, passes check_map in
    more than 90 % of the cells."""
    case = next(c for c in K.CASES if c.id == case_id)
    _, ref = K.reference(case)
    sh = K.unchecked_shares_check_map(ref)
    print(f"{case.id}: unchecked under check_map " + ", ".join(f"{k} {v:.4f}" for k, v in sh.items()))
    assert min(sh["zero"], sh["row"], sh["bin"]) > 0.90, sh


FAIR_USE = 0.05        # ten times the 0.005 .. 0.008 the restatement was measured to use


@pytest.mark.parametrize("case", [c for c in K.WHITE if _fp32_runnable(c)], ids=lambda c: c.id)
def test_white_case_is_fair_to_fp32(case):
    """The C fp32 restatement on the white scene uses at most 0.05 of the every-cell bound (the fp32
    rule whatever the case's spectrum: the restatement keeps an fp32 spectrum): scene and rule leave a
    correct fp32 implementation a factor of 20."""
    c = case.cfg
    cube, ref = K.reference(case)
    got, _, _ = CB.process(K.to_complex(cube, c.in_dtype).astype(np.complex64), None, threads=4)
    assert K.check_every_cell(dataclasses.replace(c, spectrum="f32"), got, ref, case) <= FAIR_USE


@pytest.mark.parametrize("case", WHITE_F16, ids=lambda c: c.id)
def test_white_case_is_fair_to_the_fp16_spectrum(case):
    """The fp16 format alone, applied in fp64 to the oracle's range spectrum as
    test_case_is_fair_to_the_fp16_spectrum applies it, moves no cell of a white case's map by more than
    E = fp16_row_error: what the every-cell rule adds for the format covers the format."""
    c = case.cfg
    cube, ref = K.reference(case)
    E = K.fp16_row_error(case)
    worst = 0.0
    for f in range(case.nf):
        spec = O.range_ct(K.to_complex(cube[f], c.in_dtype)) * 2.0 ** -c.range_shift
        rd = O.doppler_stage(_fp16(spec / c.n_range) * c.n_range, mti_mode=c.mti)
        m = K.ambm_f64(rd[0]) if c.magnitude == "ambm" else O.magnitude(rd, rx_axis=0)
        worst = max(worst, float((np.abs(m - ref[f]) / E[f][:, None]).max()))
    print(f"{case.id}: the format alone uses {worst:.3g} of E")
    assert worst <= 1.0


# -- a defect catalogue: what a wrong K2 would write, modelled on the oracle's stages
def _stage_map(c, spec, window=None):
    """The oracle's map [range][doppler] (fp64) of one frame's range spectrum [rx][range][chirp]; `window`:
    another Doppler window than the configuration's."""
    x = O.mti(spec, c.mti)
    w = O.window_f32(c.n_doppler).astype(np.float64) if window is None else window
    rd = np.fft.fft(x * w, axis=-1)
    return K.ambm_f64(rd[0]) if c.magnitude == "ambm" else O.magnitude(rd, rx_axis=0)


def _defects(case):
    """{name: map [frame][range][doppler] fp64} of the defects that apply to the case, each in one wave
    tile (WR range rows x NC, cfar1d.hpp DopplerGeom::WR) or one row of frame 0, away from the map's edges."""
    c = case.cfg
    cube, ref = K.reference(case)
    spec = [O.range_ct(K.to_complex(cube[f], c.in_dtype)) for f in range(case.nf)]
    for f in range(case.nf):         # the stages put together as here are the oracle
        np.testing.assert_allclose(_stage_map(c, spec[f]), ref[f], rtol=1e-12, atol=1e-9 * ref[f].max())
    nc, P = c.n_doppler, c.n_doppler // 16
    WR = 64 // P
    t = min(5, c.n_range // WR - 1)
    rows = slice(t * WR, (t + 1) * WR)
    before = slice((t - 1) * WR, t * WR)
    row = t * WR + WR // 2
    out = {}

    def put(name, tile=None, at=rows, one_row=None):
        m = ref.copy()
        if one_row is None:
            m[0, at] = tile
        else:
            m[0, row] = one_row
        out[name] = m

    put("a: one wave tile never stored", 0.0)
    put("b: the tile holds the rows of the tile before it", ref[0, before])
    if c.n_rx > 1:
        put("c: one rx missing from NCI in one tile", _stage_map(c, spec[0][:-1, rows]))
    put("d: the Doppler window one chirp late in one tile",
        _stage_map(c, spec[0][:, rows], np.roll(O.window_f32(nc).astype(np.float64), 1)))
    swapped = ref[0, row].copy()
    swapped[[nc // 2, nc // 2 + 1]] = swapped[[nc // 2 + 1, nc // 2]]
    put("e: two neighbouring Doppler bins swapped in one row", one_row=swapped)
    if c.spectrum == "s48":
        # one shared-exponent group of 4 chirps (fmcw.h FMCW_SPEC_S48; at n_range 1024 the chirps of a
        # group lie n_doppler / 16 apart) decoded with twice its exponent's scale
        s = spec[0][:, row:row + 1].copy()
        group = 7 % P + P * np.arange(4) if K.doppler_sp(c) == 4 else 4 * (nc // 8) + np.arange(4)
        s[..., group] *= 2.0
        put("f: one 4-chirp group scaled by 2, the neighbour's exponent", one_row=_stage_map(c, s)[0])
    if case.nf > 1:
        put("g: one tile taken from the other frame", ref[1, rows])
    if c.mti == 2:
        # doppler_kernel.hpp k_doppler `c >= 1 ? at(c - 1) : 0`: the canceller starts from a zero history
        s = spec[0][:, rows]
        x = O.mti(s, 2)
        x[..., 0] = s[..., 0] - s[..., -1]
        w = O.window_f32(nc).astype(np.float64)
        put("h: the canceller's history not zeroed at the first chirp", O.magnitude(np.fft.fft(x * w, axis=-1), rx_axis=0))
    return ref, out


@pytest.mark.parametrize("white_id", ["process-k2-128-f32-mti2-white", "process-k2-64-s48-strided-fast-nrx2-white"])
def test_white_scene_catches_the_defect_catalogue(white_id):
    """Numpy models of what a wrong K2 would leave in the map, on an fp32 case (64 x 128, n_rx 2, MTI 2) and
    on a strided-S48 case (1024 x 64, n_rx 2): each fails check_every_cell on the white scene.  Which of them
    check_map lets through on the base case's tone scene is printed: a record, not a requirement."""
    white = next(c for c in K.WHITE if c.id == white_id)
    base = next(c for c in K.CASES if c.id == K.WHITE_BASE[white_id])
    c = white.cfg
    assert (c.n_range, c.n_doppler, c.n_rx, c.spectrum) in ((64, 128, 2, "f32"), (1024, 64, 2, "s48"))
    ref, wrong = _defects(white)
    assert K.check_every_cell(c, ref.astype(np.float32), ref, white) <= 0.01       # float32 rounding of the oracle itself
    want = set("abcdeg") | ({"f"} if c.spectrum == "s48" else set()) | ({"h"} if c.mti == 2 else set())
    assert {n[0] for n in wrong} == want
    for name, m in wrong.items():
        with pytest.raises(AssertionError, match="beyond the bound"):
            K.check_every_cell(c, m.astype(np.float32), ref, white)
    tone_ref, tone_wrong = _defects(base)
    passed = []
    for name, m in tone_wrong.items():
        try:
            K.check_case_map(base.cfg, m.astype(np.float32), tone_ref)
            passed.append(name[0])
        except AssertionError:
            pass
    print(f"{base.id}: check_map on the tone scene lets through defects {passed or 'none'} of {sorted(n[0] for n in tone_wrong)}")
