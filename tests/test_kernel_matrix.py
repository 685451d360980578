"""CPU checks of the kernel test matrix (tests/kernel_matrix.py): the case table covers every
kernel variant the dispatch rules can reach, the rules agree with the kernels the built library
carries, and the cases' inputs are fair (a correct fp32 implementation passes them) and not
vacuous (the 1-D CFAR maps have detections at every edge the kernels treat specially, and a tie)."""
import dataclasses
import re
import subprocess

import numpy as np
import pytest

import cpu_backend as CB
import kernel_matrix as K
from test_abi import extract_code_objects

PROCESS = [c for c in K.CASES if c.group == "process"]
CFAR1D = [c for c in K.CASES if c.group == "cfar1d"]


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
                "k_range<1024,LoadI16,false,4>/cw=1"):
        assert key in covered, key
    geoms = {(c.cfg.n_range, c.cfg.n_doppler) for c in PROCESS if c.cfg.spectrum == "s48"}
    assert {(64, 64), (128, 64), (256, 64), (512, 64), (128, 128), (1024, 1024), (2048, 1024)} <= geoms
    assert any(c.cfg.n_range == 1024 and c.cfg.n_doppler == 256 and c.cfg.n_rx == 2 for c in PROCESS)


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
