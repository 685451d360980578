"""Python mirror of libfmcw.so's kernel selection, and the table of GPU cases built on it.

A helper for test_kernel_matrix.py (CPU) and test_gpu_matrix.py (GPU), not a test module.

`variants(cfg, api)` returns readable keys for every kernel instantiation and every
geometry-dependent branch inside it that the library runs for a configuration; `legal(cfg)`
mirrors validate(); `reachable()` enumerates the legal configuration space over the discrete axes
below and returns the union; `CASES` is the hand-written table of GPU cases, each at the smallest
shape that reaches its keys.  test_kernel_matrix.py holds `reachable()` against the union over
`CASES` and against the kernel symbols of the built library, so a new instantiation that no case
runs fails the CPU suite.

Every rule cites the source it restates (paths relative to fpga-fmcw-radar-processor_amd/csrc).
What the mirror leaves out, because it selects no other code: FMCW_WIN_NONE (the Hamming kernels
with a table of ones, fmcw_api.hip window_table), range_shift, chunking and the detection scratch.

The integer (RTL-compatible) datapath is an axis of its own (cases "process-int-*"): the canceller
on the spectrum's 16-bit words (FMCW_COMPAT_MTI, or the Q15 window with MTI on: key ".../words")
and the integer Doppler window on the canceller's output (".../words+q15d") are runtime branches
of the twelve generic MTI kernels, whose lane geometry differs at every Doppler size.  Their cases
run int16 cubes that clip nowhere ("int_clean") and cubes that clip at every stage ("int_sat"), and
test_gpu_matrix.test_integer_path holds the status words to the oracle's counts (integer_counts).

The 2-D CFAR (K3a / K3b / K3c, cfar2d.hpp) is mirrored down to the branches its window geometry,
parameters, shape and strip length select (`cfar2d_select`), and runs as a stage of its own (group
"cfar2d") on crafted maps (`cfar2d_layout`).  The strip length the cost model picks (cfar2d_steps 0)
depends on the CU count and has no key; one case per Doppler size and window runs it.

The persistent loops of K1, K2, k_cfar1d and K3 run one iteration per workgroup at these shapes; the
cases "*-loop-g<grid>" repeat a case of the table under capped grids (Case.grid, fmcw_set_param's
FMCW_PARAM_GRID_*) and claim a "<key>/loop" twin only where `loops` counts three iterations or more.

`WHITE` is a derived table: for every K1 / K2 key with a twin, the twin, and the AMBM branch, the first
whole-path case of `CASES` that claims it, once more on white full-scale noise ("<id>-white"), where
`check_every_cell` holds every cell of the map to 1e-4 of the rms of its own range row.
"""
from __future__ import annotations

import dataclasses
import functools
import itertools
from dataclasses import dataclass

import numpy as np

N_RANGE = (64, 128, 256, 512, 1024, 2048, 4096, 8192)     # dispatch.hpp / inst_range.hip R_()
N_DOPPLER = (32, 64, 128, 256, 512, 1024)                  # inst_doppler.hip doppler_info D_()
N_RX = (1, 2, 3)                                           # one, even, odd (the rx loop of k_doppler)
IN_DTYPES = ("f32", "f16", "i16")
WINDOWS = ("hamming", "q15_rtl")
SPECTRA = ("f32", "f16", "s48")
MTI = (0, 2, 3)
MAGNITUDES = ("abs", "ambm")
MAP_KINDS = ("linear", "db")
# 1-D CFAR parameter sets (ref, guard, rank, alpha): the reference, the multi-group screen
# (need = 16 - rank > 4), need = 1, and runtime geometries: a maximal window at NC = 32, one wider
# than the 16-cell halo, the largest rank of a 16-ref window, and the existing (6, 1, 9, 3.0)
CFAR1D_SETS = ((8, 2, 12, 4.0), (8, 2, 0, 4.0), (8, 2, 7, 4.0), (8, 2, 11, 4.0), (8, 2, 11, 1.5),
               (8, 2, 7, 1.5), (8, 2, 15, 4.0), (12, 3, 18, 4.0), (20, 3, 30, 4.0), (16, 0, 31, 4.0),
               (6, 1, 9, 3.0))
# 2-D CFAR windows (ref_range, guard_range, ref_doppler, guard_doppler): the reference (n_ref 128),
# n_ref 54, n_ref 64 without guards, n_ref 112 (above 64, no power of two), hr = 0 with hd = 21
# beyond the halo, hd = 0 (n_ref 6), 2 hd + 1 = 31 (maximal at NC = 32), 128 cells along Doppler
# only, hr = 8 (>= TR at NC >= 512)
CFAR2D_SETS = ((4, 1, 4, 2), (2, 1, 3, 1), (2, 0, 6, 0), (3, 0, 5, 3), (0, 0, 20, 1), (3, 1, 0, 0),
               (1, 0, 14, 1), (0, 0, 64, 0), (7, 1, 1, 0))
CFAR2D_RANK_PCT = (0, 75, 100)
CFAR2D_OVERRIDE = (0, 3)
CFAR2D_STEPS = (1, 3, 5)

SP_NAME = {0: "F32", 1: "F16", 2: "S48", 4: "S48S", 5: "S48PS"}   # spectrum.hpp SP_*
LOAD = {"f32": "LoadF32", "f16": "LoadF16", "i16": "LoadI16"}
MH = 16                                                            # cfar1d.hpp MH: halo cells per side
RANGE_SINGLE, RANGE_SEQ, RANGE_PX = 0, 2, 3                        # dispatch.hpp RangeKind


@dataclass(frozen=True)
class Cfg:
    n_range: int = 64
    n_doppler: int = 32
    n_rx: int = 1
    in_dtype: str = "f32"
    window: str = "hamming"
    spectrum: str = "f32"
    mti: int = 0
    magnitude: str = "abs"
    map_kind: str = "linear"
    cfar: str = "none"                       # "none", "os1d", "os2d"
    cfar1d: tuple = (8, 2, 12, 4.0)          # ref, guard, rank, alpha
    cfar2d: tuple = (4, 1, 4, 2)             # ref_range, guard_range, ref_doppler, guard_doppler
    compat_cfar: bool = False
    range_shift: int = 0
    cfar2d_rank_pct: int = 75
    cfar2d_scales: tuple = (2, 4, 6)         # scale_min, scale_nom, scale_max
    cfar2d_override: int = 0
    compat_mti: bool = False                 # FMCW_COMPAT_MTI: the canceller on 16-bit words


# ---- validate() ---------------------------------------------------------------------------
def illegal_reason(c: Cfg):
    """plan.hip validate(), in its order (each arm cites the message validate fails with); None when the
    configuration is legal."""
    if c.n_range not in N_RANGE:                                   # "n_range=%u: must be a power of two in [64, 8192]"
        return "n_range"
    if c.n_doppler not in N_DOPPLER:                               # "n_doppler=%u: must be a power of two in [32, 1024]"
        return "n_doppler"
    if not 1 <= c.n_rx <= 64:                                      # "n_rx=%u: must be in [1, 64]"
        return "n_rx"
    if c.window == "q15_rtl" and c.in_dtype != "i16":              # "window Q15_RTL windows int16 ADC words: needs in_dtype I16"
        return "q15 needs i16"
    if c.magnitude == "ambm" and c.n_rx != 1:                      # "mag_mode AMBM is defined for n_rx == 1 only"
        return "ambm needs n_rx 1"
    if range_T(c.n_range) > c.n_doppler:                           # "n_doppler=%u smaller than the range kernel's chirp group"
        return "n_doppler below the chirp group"
    if c.cfar == "os1d":
        ref, guard, rank, alpha = c.cfar1d
        if ref < 1 or rank >= 2 * ref:                             # "1-D CFAR: need ref >= 1 and rank < 2*ref"
            return "rank"
        if 2 * (ref + guard) + 1 > c.n_doppler:                    # "1-D CFAR window wider than n_doppler"
            return "1-D window wider than n_doppler"
        if not alpha > 0:                                          # "1-D CFAR alpha must be > 0"
            return "alpha"
        if c.compat_cfar and not (alpha == int(alpha) and alpha <= 16384):   # "compat CFAR: alpha is the integer SCALING_MULT (1..16384)"
            return "compat alpha"
    elif c.cfar == "os2d":
        if c.cfar2d_rank_pct > 100:                                # "2-D CFAR: rank_pct %u > 100"
            return "2-D rank_pct"
        if max(c.cfar2d) > 64:                                     # "2-D CFAR window extents out of range"
            return "2-D window extents"
        hr, _, hd, _, n_ref, _ = cfar2d_geom(c)
        if not 1 <= n_ref <= 128:                                  # "2-D CFAR: %d reference cells (supported 1..128)"
            return "2-D n_ref"
        if 2 * hd + 1 > c.n_doppler:                               # "2-D CFAR window wider than n_doppler"
            return "2-D window wider than n_doppler"
        if c.cfar2d_override > 7:                                  # "scale_override is a 3-bit port (0..7)"
            return "2-D scale override"
        if cfar2d_smem(c) > 160 * 1024:                            # "2-D CFAR range extent too large for LDS"
            return "2-D range extent too large for LDS"
    if c.compat_mti and c.mti == 0:                                # "compat MTI needs mti_mode 2 or 3"
        return "compat MTI needs MTI on"
    if c.range_shift > 13:                                         # "range_shift=%u: must be in [0, 13]"
        return "range_shift"
    if c.spectrum == "s48":
        if c.n_doppler < 64:                                       # "spectrum_dtype S48 needs n_doppler >= 64"
            return "s48 needs n_doppler >= 64"
        if c.mti != 0 or c.window == "q15_rtl":                    # "spectrum_dtype S48 is defined with MTI off and an fp32 window (not Q15_RTL)"
            return "s48 needs MTI off and an fp32 window"
    if c.spectrum == "f16" and c.compat_mti:                       # "compat MTI is defined on the fp32 spectrum (spectrum_dtype F16)"
        return "compat MTI needs the fp32 spectrum"
    if c.spectrum == "f16" and c.window == "q15_rtl":              # "window Q15_RTL is defined on the fp32 spectrum (spectrum_dtype F16)"
        return "q15 needs the fp32 spectrum"
    return None


def legal(c: Cfg) -> bool:
    return illegal_reason(c) is None


# ---- K1 -----------------------------------------------------------------------------------
def range_T(n: int) -> int:
    """range_kernels.hpp RangeGeom<N>::T (= SqGeom::T and the 2 of inst_range.hip range_px)."""
    return 16 if n <= 128 else 8 if n <= 512 else 4 if n == 1024 else 2


@functools.lru_cache(maxsize=None)
def range_select(n: int, in_dtype: str, window: str, spectrum: str):
    """inst_range.hip range_info with want = kRangePx (the release library's preference,
    plan.hpp PlanPrefs::k1_want): (family, symbol, SP) or None where range_fn returns nullptr."""
    q15 = window == "q15_rtl"
    ld = LOAD[in_dtype]
    if not q15 and spectrum in ("f32", "s48"):                     # range_info: the pair kernels, `!q15 && (spec == FMCW_SPEC_F32 || spec == FMCW_SPEC_S48)`
        sp = 5 if spectrum == "s48" else 0                         # inst_range.hip range_px / range_sq: SP_S48PS or SP_F32
        if n == 8192:                                              # range_info `want >= kRangePx && n == 8192`, range_px_t
            return RANGE_PX, f"k_range_px<fmcw::{ld}, 4, {6 if sp == 5 else 4}, {sp}>", sp
        if n == 4096:                                              # range_info `want >= kRangeSeq && n == 4096`, SqPick<4096>
            return RANGE_SEQ, f"k_range_sq<4096, fmcw::{ld}, 16, 1, 3, {sp}>", sp
    if spectrum == "s48":                                          # range_fn: the S48 form by RangeGeom<N>::T
        if q15 or n > 2048:
            return None
        T = range_T(n)
        sp = 4 if T == 4 else 5 if T == 2 else 2
    else:
        sp = 1 if spectrum == "f16" else 0                         # range_fn: SP_F16 or SP_F32
    return RANGE_SINGLE, f"k_range<{n}, fmcw::{ld}, {'true' if q15 else 'false'}, {sp}>", sp


# ---- K2 -----------------------------------------------------------------------------------
def k2_fast(c: Cfg) -> bool:
    """plan.hip k2_fast."""
    ref, guard, rank, _ = c.cfar1d
    cfar_ok = c.cfar != "os1d" or (ref == 8 and guard == 2 and 2 * ref - rank <= 4 and not c.compat_cfar)
    return (c.mti == 0 and c.magnitude != "ambm" and c.map_kind != "db" and c.window != "q15_rtl"
            and cfar_ok)


def k2_prefetch(nc: int, mti: int) -> int:
    """doppler_kernel.hpp k2_prefetch."""
    return 0 if mti else 16 if nc <= 256 else 8 if nc == 512 else 0


def doppler_sp(c: Cfg) -> int:
    """inst_doppler.hip doppler_info and dispatch.hpp s48_form."""
    if c.spectrum == "f16":
        return 1
    if c.spectrum == "s48":
        T = range_T(c.n_range)
        return 5 if T == 2 else 4 if T == 4 else 2
    return 0


def cfar1d_branch(c: Cfg) -> str:
    """cfar1d.hpp cfar1d_dispatch."""
    ref, guard, rank, _ = c.cfar1d
    if c.compat_cfar:
        return "rtl"
    if ref == 8 and guard == 2:
        return "8,2,one-group" if 2 * ref - rank <= 4 else "8,2,multi-group"
    return "runtime"


def cfar1d_keys(c: Cfg, where: str) -> set:
    """The 1-D CFAR branch a wave tile takes, tagged by the kernel it runs in (`where`)."""
    nc = c.n_doppler
    ref, guard, _, _ = c.cfar1d
    br = cfar1d_branch(c)
    keys = {f"cfar1d<{nc},{br}>/{where}"}
    if br == "runtime":
        # cfar1d.hpp cfar1d_wave<NC, 0, 0> (REF == 0 arms): offsets wrap with & (NC - 1); beyond the MH-cell halo only
        # this wrap keeps them inside the row, and at 2 (ref + guard) + 1 = NC - 1 the two sides meet
        if ref + guard > MH:
            keys.add(f"cfar1d<{nc},runtime>/window>halo/{where}")
        if 2 * (ref + guard) + 1 == nc - 1:
            keys.add(f"cfar1d<{nc},runtime>/maximal/{where}")
    return keys


def cfar2d_geom(c: Cfg):
    """plan.hip cfar2_args: (hr, gr, hd, gd, n_ref, rank)."""
    rr, gr, rd, gd = c.cfar2d
    hr, hd = rr + gr, rd + gd
    n_ref = (2 * hr + 1) * (2 * hd + 1) - (2 * gr + 1) * (2 * gd + 1)        # cfar2_args a.n_ref
    rank = min(n_ref * c.cfar2d_rank_pct // 100, n_ref - 1)                   # cfar2_args a.rank
    return hr, gr, hd, gd, n_ref, rank


def cfar2d_TR(nc: int) -> int:
    """cfar2d.hpp Cfar2DGeom<NC>::TR: CUT rows of a workgroup step, WPB 4 x WR = 1024 / NC."""
    return 4096 // nc


def cfar2d_lv(c: Cfg) -> bool:
    """inst_cfar2.hip lv_window."""
    hr, gr, hd, gd, _, _ = cfar2d_geom(c)
    return (hd, gd, hr, gr) == (6, 2, 5, 1)


def cfar2d_smem(c: Cfg) -> int:
    """The LDS bytes of the K3a kernel cfar2_info picks (inst_cfar2.hip info_t)."""
    nc = c.n_doppler
    hr = cfar2d_geom(c)[0]
    if cfar2d_lv(c):
        if nc == 1024:      # cfar2d.hpp LvGeom::SMEM, HR 5: NR x ROWB + (HIST + CAPB + 2 CAPT) x 4
            return (cfar2d_TR(nc) + 2 * 5 + 1) * (2 * (nc + 16) + nc // 2) + (144 + 192 + 2 * 64) * 4
        hr = 5
    # cfar2d.hpp cfar2d_smem_bytes: (TR + 2 hr) x (RB + 2 KRS) + kCfar2dList x 4
    return (cfar2d_TR(nc) + 2 * hr) * ((nc + 2 * MH + 16) + 2 * (nc + 2 * MH)) + (2 * 256 + 16) * 4


def cfar2d_strips(n_range: int, nc: int, steps: int):
    """launch.hip launch_cfar (tpf, n_strips) and the strip loop of k_cfar2d (cfar2d.hpp `t_beg`, `t_end`;
    k_cfar2d_lv the same): [(strip index within the frame, its steps)] for a strip length."""
    tpf = -(-n_range // cfar2d_TR(nc))                # workgroup steps per frame
    s = min(steps, tpf)
    return [(i, min(s, tpf - i * s)) for i in range(-(-tpf // s))]


def cfar2d_select(c: Cfg, steps: int = 0):
    """inst_cfar2.hip cfar2_info: [(key, symbol)], then (key, None) for every branch of
    cfar2d.hpp the configuration, the shape and the strip length `steps` (0: the cost model's
    choice, which depends on the CU count and is not mirrored) take, tagged with its kernel."""
    nc = c.n_doppler
    hr, gr, hd, gd, n_ref, rank = cfar2d_geom(c)
    lv = cfar2d_lv(c)                                              # inst_cfar2.hip lv_window
    rules = lv and nc == 1024                                      # rules_kernel (info_t static_assert N == 1024)
    if rules:
        a = f"k_cfar2d_lv<1024, 5, 1, {'true' if c.compat_cfar else 'false'}>"
    elif lv:
        a = f"k_cfar2d<{nc}, 6, 2, 5, 1>"                          # info_t, lv without rules_kernel: k_cfar2d<N, 6, 2, 5, 1>
    else:
        a = f"k_cfar2d<{nc}, 0, 0, 0, 0>"                          # info_t default: k_cfar2d<N, 0, 0>
    out = [(s.replace(" ", ""), s) for s in (a, f"k_cfar2d_decide<{nc}>", f"k_cfar2d_emit<{nc}>")]
    ka, kb, kc = (k for k, _ in out)
    keys = []
    if c.compat_cfar:
        if not rules:                # k_cfar2d_lv carries compat in its symbol (CMP)
            keys.append(f"{ka}/compat")                            # cfar2d.hpp k_cfar2d `a.compat ? q17... : nonneg...` (q17 cells)
        keys.append(f"{kb}/compat")                                # k_cfar2d_decide `a.compat` (cfar2d_decide_run CMP: integer mean and brackets)
        keys.append(f"{kc}/compat")                                # k_cfar2d_emit `dd.mag = a.compat ? q17(v) : nonneg(v)`
    if c.cfar2d_override:
        keys.append(f"{ka}/override")                              # `a.override_` in cfar2d_exact_a (k_cfar2d) and `s2ok` (k_cfar2d_lv)
        keys.append(f"{kb}/override")                              # cfar2d_decide_run `if (!a.override_)`: no mean, no bracket
    elif not c.compat_cfar:                                        # cfar2d_decide_run fl(sum / n): `inv_n`, `n_pow2`
        keys.append(f"{kb}/n_ref={'pow2' if n_ref & (n_ref - 1) == 0 else 'div'}")
    if n_ref <= 64:
        keys.append(f"{kb}/n_ref<=64")                             # cfar2d_decide_run `okb` is never true
    if rank == 0:                                                  # `need = a.n_ref - a.rank` (k_cfar2d, k_cfar2d_lv); wave_select_kth k = 0
        keys += [f"{ka}/rank=0", f"{kb}/rank=0"]
    if rank == n_ref - 1:                                          # need = 1; select k = n_ref - 1
        keys += [f"{ka}/rank=n_ref-1", f"{kb}/rank=n_ref-1"]
    if not lv:                       # runtime geometry of k_cfar2d<NC,0,0,0,0>
        if hd > MH:                                                # cfar2d_screen7_generic `pm`, cfar2d_exact_a: wrap with & (NC - 1)
            keys.append(f"{ka}/window>halo")
        if 2 * hd + 1 == nc - 1:                                   # the two Doppler sides meet at the wrap
            keys.append(f"{ka}/maximal")
        if hr == 0:                                                # k_cfar2d `nr = TR + 2 * a.hr` == TR, every row `tested`
            keys.append(f"{ka}/hr=0")
        if hd == 0:                                                # cfar2d_screen7_generic `nps` == 0: the screen counts nothing
            keys.append(f"{ka}/hd=0")
        if hr >= cfar2d_TR(nc):                                    # the ring turn (k_cfar2d `rr.base +=`) moves fewer rows than a halo
            keys.append(f"{ka}/hr>=TR")
    if c.n_range < cfar2d_TR(nc):                                  # k_cfar2d `n_wt` < WPB, `has_tile`
        keys.append(f"{ka}/step=partial")
    if steps:
        strips = cfar2d_strips(c.n_range, nc, steps)
        for i, n in strips:
            if n == 1:                                             # k_cfar2d `first` == `last`: no turn, no prefetch
                keys.append(f"{ka}/strip=one-step")
            else:                                                  # k_cfar2d `up` (kK3AltDir): the ring turn `rr.base +=`, the prefetch `if (!last)`
                keys.append(f"{ka}/strip={'up' if i & 1 else 'down'}")
        if strips[-1][1] < strips[0][1]:                           # k_cfar2d `t_end = min(t_beg + steps, wg_per_frame)`
            keys.append(f"{ka}/strip=short-last")
    return out + [(k, None) for k in keys]


def select(c: Cfg, api: str = "process", steps: int = 0):
    """[(key, kernel symbol or None)] for one entry point: "process" (fmcw_enqueue), "range_ct"
    (fmcw_range_ct) or "cfar" (fmcw_cfar; `steps`: the cfar2d_steps parameter)."""
    out = []
    nc = c.n_doppler
    if api == "range_ct":
        # plan.hip build_plan k1_stage (fmcw_range_ct): the fp32-spectrum K1 whatever spectrum_dtype,
        # launched with no fused Doppler weight
        _, sym, sp = range_select(c.n_range, c.in_dtype, c.window, "f32")
        return [(sym.replace("fmcw::", "").replace(" ", "") + "/cw=0", sym)]
    if api == "cfar":
        if c.cfar == "os1d":                                       # launch.hip launch_cfar
            out.append((f"k_cfar1d<{nc}>", f"k_cfar1d<{nc}>"))
            out += [(k, None) for k in cfar1d_keys(c, "stage")]
        elif c.cfar == "os2d":
            out += cfar2d_select(c, steps)
        return out
    # ---- fmcw_api.hip fmcw_enqueue
    sel = range_select(c.n_range, c.in_dtype, c.window, c.spectrum)
    if sel is None:
        return []
    _, sym, _ = sel
    cw = int(c.mti == 0 and c.window != "q15_rtl")                  # fmcw_api.hip `chirp_w = c.mti_mode == FMCW_MTI_OFF && !p.q15 ? h->win_d : nullptr`
    out.append((sym.replace("fmcw::", "").replace(" ", "") + f"/cw={cw}", sym))
    fast = k2_fast(c)
    sp = doppler_sp(c)
    if sp >= 2 and (nc < 64 or c.mti != 0):                        # inst_doppler_s48.hip dfn_t
        return []
    T = range_T(c.n_range)
    P = nc // 16                                                   # cfar1d.hpp DopplerGeom::P
    WR, WPB = 64 // P, 4                                           # DopplerGeom::WR, ::WPB
    npf = k2_prefetch(nc, c.mti)
    if npf == 0:
        addr = ""
    elif sp in (4, 5):
        addr = "/strided"                                          # doppler_kernel.hpp k_doppler prefetch, the strided-S48 arm
    elif P & (T - 1) == 0:
        addr = "/uniform"                                          # k_doppler prefetch `(P & (T - 1)) == 0`: the uniform arm
    else:
        addr = "/per-point"                                        # k_doppler prefetch, the last arm: an address per point
    kind = "FAST" if fast else "GEN"
    out.append((f"k_doppler<{nc},mti={c.mti},{SP_NAME[sp]},{kind}>/pf={npf}{addr}",
                f"k_doppler<{nc}, {c.mti}, {sp}, {'true' if fast else 'false'}>"))
    nbytes = 6 if sp >= 2 else 8
    if WPB * WR * nbytes * T < 128:                                # k_doppler `xcd`
        out.append((f"k_doppler/xcd-remap<NC={nc},B={nbytes},T={T}>", None))
    tiles = c.n_range // WR
    out.append((f"k_doppler<{nc}>/tile-order={'grouped' if tiles % WPB == 0 else 'frame-minor'}", None))   # k_doppler `grp`
    if c.n_rx > 1:                                                 # k_doppler: the rx loop, the prefetch site `same ? rx + 1 : 0`
        out.append((f"k_doppler/nci<pf={npf},{SP_NAME[sp]}>", None))
        if c.n_rx % 2:
            out.append(("k_doppler/nci/odd-nrx", None))
    if not fast:                                                   # runtime branches of the generic kernel
        if c.magnitude == "ambm":
            out.append((f"k_doppler<{nc},{SP_NAME[sp]},GEN>/ambm", None))        # k_doppler `mag_mode == FMCW_MAG_AMBM`, `ambm`
        if c.map_kind == "db":
            out.append((f"k_doppler<{nc},{SP_NAME[sp]},GEN>/db", None))          # k_doppler `!FAST && db_map`
        if c.window == "q15_rtl":
            out.append((f"k_doppler<{nc},{SP_NAME[sp]},GEN>/q15d", None))        # k_doppler `q15d`: the wv_d load, win_q15c
        if c.mti and (c.compat_mti or c.window == "q15_rtl"):
            # the canceller on 16-bit words: neighbours re-read and re-quantised, saturating output
            out.append((f"k_doppler<{nc},mti={c.mti},{SP_NAME[sp]},GEN>/words", None))        # k_doppler `words`: q16c_count .. sat16c_count
            if c.window == "q15_rtl":        # the integer window on the canceller's output: win_q15c after sat16c_count
                out.append((f"k_doppler<{nc},mti={c.mti},{SP_NAME[sp]},GEN>/words+q15d", None))
    if c.cfar == "os1d":                                           # k_doppler `cf.enabled`: cfar1d_wave<NC, 8, 2, true> / cfar1d_dispatch
        out += [(k, None) for k in cfar1d_keys(c, "fused-fast" if fast else "fused-generic")]
    elif c.cfar == "os2d":                                         # launch.hip launch_cfar from fmcw_enqueue
        out += cfar2d_select(c)
    return out


def variants(c: Cfg, api: str = "process", steps: int = 0) -> set:
    return {k for k, _ in select(c, api, steps)}


def range_family(c: Cfg, api: str = "process") -> int:
    """FMCW_INFO_RANGE_KERNEL: the family fmcw_create picked with the handle's spectrum (fmcw_api.hip fmcw_create)."""
    return range_select(c.n_range, c.in_dtype, c.window, c.spectrum)[0]


# ---- the persistent loops ------------------------------------------------------------------
# K1, K2, k_cfar1d and K3a stride over their units with `for (g = blockIdx.x; g < n; g += gridDim.x)`
# (the `g += gridDim.x` loops of k_range, k_range_sq, k_range_px, the `tile +=` loops of k_cfar1d, k_doppler and
# the strip loops of k_cfar2d, k_cfar2d_lv); K3b / K3c over candidates and wave tiles per wave (cfar2d.hpp
# cfar2d_decide_run, k_cfar2d_emit `nw`).  The grids are occupancy x CUs (launch.hip
# device_grids; 1024 for K3b / K3c), so at the shapes of this table a workgroup runs one iteration
# unless the grid is capped (fmcw_set_param FMCW_PARAM_GRID_*, Case.grid).  A key "<key>/loop" says: a
# case ran that kernel so that its busiest workgroup went through the loop at least LOOP_MIN times.
LOOP_MIN = 3     # iteration 2 is the first to consume a prefetch issued inside the loop, iteration 3
#                  the first that both consumes one and has issued one before it
LOOP_GRIDS = (1, 2, 3, 16)
MAX_CELLS = 2048 * 1024      # no case is larger than the "fast-xcd" shape: 2048 x 1024 x 1 frame


def loopable(key: str, sym) -> bool:
    """Keys that get a "/loop" twin: those that carry a kernel symbol, and K2's NCI, XCD-remap and
    tile-order keys (the rx loop carries the prefetch into the next tile at k_doppler's prefetch site;
    xcd_block_id and tile_fl decide which units a workgroup strides over)."""
    return sym is not None or key.startswith(("k_doppler/nci<", "k_doppler/xcd-remap<")) or "/tile-order=" in key


def loop_kernel(key: str) -> str:
    """The kernel whose loop a loopable key belongs to."""
    for prefix, kern in (("k_range", "k1"), ("k_doppler/xcd-remap<", "xcd"), ("k_doppler", "k2"),
                         ("k_cfar1d<", "cfar1d"), ("k_cfar2d_decide<", "k3b"), ("k_cfar2d_emit<", "k3c"),
                         ("k_cfar2d", "k3a")):
        if key.startswith(prefix):
            return kern
    raise KeyError(key)


def tiles_frame(c: Cfg) -> int:
    """Wave tiles of a frame: n_range / WR, WR = 64 / P rows of P = NC / 16 lanes (cfar1d.hpp DopplerGeom::P, ::WR;
    plan.hip tiles_frame)."""
    return c.n_range // (64 // (c.n_doppler // 16))


def k1_units(c: Cfg, nf: int) -> int:
    """launch.hip launch_range: n_groups = nf * n_rx * (n_doppler / T) chirp groups per K1 launch."""
    return nf * c.n_rx * (c.n_doppler // range_T(c.n_range))


def tile_units(c: Cfg, nf: int) -> int:
    """launch.hip tile_grid (K2 and k_cfar1d): ceil(nf * tiles_frame / WPB) workgroup steps, WPB = 4."""
    return -(-nf * tiles_frame(c) // 4)


def k3a_units(c: Cfg, nf: int, steps: int) -> int:
    """launch.hip launch_cfar `n_strips`: nf * ceil(tpf / steps) strips, tpf = ceil(tiles_frame / 4)."""
    return nf * len(cfar2d_strips(c.n_range, c.n_doppler, steps))


def k3c_units(c: Cfg, nf: int) -> int:
    """Wave tiles of a K3 launch (at most: k_cfar2d_emit takes those with candidates, cfar2d.hpp `cands.ctr[1]`),
    shared by the 4 waves of each workgroup."""
    return nf * tiles_frame(c)


def wg_units(units: int, grid: int):
    """The units each workgroup of a launch takes, in its order: the launch sites bound the grid by
    the unit count (launch.hip tile_grid, launch_range, launch_cfar), workgroup b takes b, b + grid, ..."""
    g = min(units, grid)
    return [list(range(b, units, g)) for b in range(g)]


def busiest(units: int, grid: int) -> int:
    """Iterations of the busiest workgroup; the last of them has no next unit (the loops end)."""
    return max(map(len, wg_units(units, grid)), default=0)


def k3a_walk(c: Cfg, nf: int, steps: int, grid: int):
    """Per workgroup, the strips it takes as (frame, "down" / "up" / "one-step"): strip g is strip
    g / nf of frame g % nf, odd strips walk upwards (cfar2d.hpp k_cfar2d / k_cfar2d_lv strip loop)."""
    per_frame = cfar2d_strips(c.n_range, c.n_doppler, steps)
    out = []
    for mine in wg_units(nf * len(per_frame), grid):
        out.append([(g % nf, "one-step" if per_frame[g // nf][1] == 1 else "up" if (g // nf) & 1 else "down")
                    for g in mine])
    return out


def k3a_turns(walk) -> bool:
    """The K3a rule: some workgroup runs a down strip right after an up strip and an up strip right
    after a down strip, on the LDS the other left behind; or, where every strip is one step (no
    direction), strips of two different frames one after the other."""
    for w in walk:
        pairs = list(zip(w, w[1:]))
        if all(d == "one-step" for _, d in w):
            if any(a[0] != b[0] for a, b in pairs):
                return True
        elif (any(a[1] == "up" and b[1] == "down" for a, b in pairs)
              and any(a[1] == "down" and b[1] == "up" for a, b in pairs)):
            return True
    return False


def launch_frames(nf: int, chunk_frames: int):
    """Frames of each K1 / K2 launch of one fmcw_process call (fmcw_api.hip, the `f0 += p.chunk` loop); the auto chunk
    holds every case of this table whole."""
    ch = chunk_frames or nf
    return [min(ch, nf - f0) for f0 in range(0, nf, ch)]


def loops(group: str, c: Cfg, nf: int, grid: int, steps: int = 0, chunk_frames: int = 0) -> dict:
    """{kernel: its busiest workgroup's iterations under a cap of `grid` workgroups} for the kernels
    whose "/loop" keys a case may claim (at least LOOP_MIN in every launch of the call; "xcd" also
    needs a launch grid that is a multiple of 8 and not 8 itself, else xcd_block_id is the identity:
    (b & 7) * (grid >> 3) + (b >> 3) = b at grid 8; "k3a" also k3a_turns).  K3b's count depends on the data: a case claims it with its grid, and
    test_kernel_matrix holds the oracle's detections of that case to 3 x 4 x grid."""
    out = {}
    if not grid:
        return out
    if group == "range":
        out["k1"] = busiest(k1_units(c, nf), grid)
    if group in ("process", "cfar1d"):
        per = launch_frames(nf, chunk_frames)
        out["k1"] = min(busiest(k1_units(c, n), grid) for n in per)
        out["k2"] = min(busiest(tile_units(c, n), grid) for n in per)
        if all(min(tile_units(c, n), grid) % 8 == 0 and min(tile_units(c, n), grid) > 8 for n in per):
            out["xcd"] = out["k2"]
    if group == "cfar1d":
        out["cfar1d"] = busiest(tile_units(c, nf), grid)
    if group == "cfar2d" and steps:
        if k3a_turns(k3a_walk(c, nf, steps, grid)):
            out["k3a"] = busiest(k3a_units(c, nf, steps), grid)
        out["k3b"] = LOOP_MIN
        out["k3c"] = -(-k3c_units(c, nf) // (4 * grid))
    return {k: n for k, n in out.items() if n >= LOOP_MIN}


def _cfar_options():
    yield "none", CFAR1D_SETS[0], CFAR2D_SETS[0], False
    for p in CFAR1D_SETS:
        yield "os1d", p, CFAR2D_SETS[0], False
    yield "os1d", CFAR1D_SETS[0], CFAR2D_SETS[0], True
    for w in CFAR2D_SETS[:2]:        # the whole path's two windows; cfar2d_reachable() has the rest
        for compat in (False, True):
            yield "os2d", CFAR1D_SETS[0], w, compat


def cfar2d_shape(nc: int) -> int:
    """n_range of the multi-step 2-D CFAR shape at a Doppler size: 8 steps, at least 64 rows."""
    return max(64, 8 * cfar2d_TR(nc))


def cfar2d_reachable():
    """{key: symbol or None} of fmcw_cfar's 2-D CFAR over the windows, ranks, overrides and strip
    lengths above, at the multi-step shape and at n_range 64 (a partial step at NC = 32).  K3 sees
    nothing of the K1 / K2 axes, so it is enumerated on its own."""
    found = {}
    for nc in N_DOPPLER:
        for ns in sorted({64, cfar2d_shape(nc)}):
            for w, pct, ovr, compat in itertools.product(CFAR2D_SETS, CFAR2D_RANK_PCT, CFAR2D_OVERRIDE,
                                                         (False, True)):
                c = Cfg(n_range=ns, n_doppler=nc, window="none", cfar="os2d", cfar2d=w, compat_cfar=compat,
                        cfar2d_rank_pct=pct, cfar2d_override=ovr)
                if illegal_reason(c):
                    continue
                for steps in (0,) + CFAR2D_STEPS:
                    found.update(select(c, "cfar", steps))
    return found


@functools.lru_cache(maxsize=None)
def reachable_with_symbols():
    """{key: symbol or None} over every legal configuration of the axes above and all three
    entry points."""
    found = {}
    opts = list(_cfar_options())
    for ns, nc, nrx, dt, win, sp, mti, mag, mk in itertools.product(
            N_RANGE, N_DOPPLER, N_RX, IN_DTYPES, WINDOWS, SPECTRA, MTI, MAGNITUDES, MAP_KINDS):
        if illegal_reason(Cfg(ns, nc, nrx, dt, win, sp, mti, mag, mk)):
            continue
        for kind, p1, p2, compat in opts:
            for cm in (False, True) if mti else (False,):
                c = Cfg(ns, nc, nrx, dt, win, sp, mti, mag, mk, kind, p1, p2, compat, compat_mti=cm)
                if illegal_reason(c):
                    continue
                sel = select(c, "process")
                if not sel:                   # plan.hip build_plan: "no kernel for this configuration"
                    continue
                found.update(sel)
                found.update(select(c, "range_ct"))
                found.update(select(c, "cfar"))
    found.update(cfar2d_reachable())
    # every configuration can be run with enough frames under a capped grid: all the twins are reachable
    found.update({k + "/loop": None for k, sym in list(found.items()) if loopable(k, sym)})
    return found


def reachable() -> set:
    return set(reachable_with_symbols())


# Kernel instantiations the library carries but no legal configuration runs.
UNREACHABLE = {}
for _n in (4096, 8192):
    for _ld in LOAD.values():
        UNREACHABLE[f"k_range<{_n}, fmcw::{_ld}, false, 0>"] = \
            "the release library prefers k_range_sq / k_range_px here (FMCW_LAB builds select it with FMCW_K1)"
for _n in N_RANGE:
    UNREACHABLE[f"k_range<{_n}, fmcw::LoadI16, true, 1>"] = \
        "validate() rejects the Q15 window on the fp16 spectrum; range_fn_t instantiates both window arms"
for _n, _sp in ((64, 2), (128, 2), (256, 2), (512, 2), (1024, 4), (2048, 5)):
    UNREACHABLE[f"k_range<{_n}, fmcw::LoadI16, true, {_sp}>"] = \
        "validate() rejects the Q15 window on the S48 spectrum; range_fn_t instantiates both window arms"


# ---- the case table -----------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    id: str
    group: str            # "range" (fmcw_range_ct), "process" (whole path), "cfar1d" (stage + fused),
    cfg: Cfg              # "cfar2d" (stage)
    nf: int = 2
    recipe: str = "random_target"     # synth.frames recipe; "uniform": white full-scale noise
    seed: int = 1234
    steps: int = 0                    # the cfar2d_steps parameter (0: the cost model)
    chunk_frames: int = 0             # fmcw_config.chunk_frames (0: the library's choice)
    grid: int = 0                     # 0: the library's grids; g > 0: all five FMCW_PARAM_GRID_* caps set to g

    def selected(self):
        if self.group == "range":
            return select(self.cfg, "range_ct")
        if self.group == "cfar2d":
            return select(self.cfg, "cfar", self.steps)
        if self.group == "cfar1d":
            return select(self.cfg, "cfar") + select(self.cfg, "process")
        return select(self.cfg, "process")

    def loops(self) -> dict:
        return loops(self.group, self.cfg, self.nf, self.grid, self.steps, self.chunk_frames)

    def keys(self) -> set:
        sel = self.selected()
        looping = self.loops()
        return {k for k, _ in sel} | {k + "/loop" for k, sym in sel if loopable(k, sym) and loop_kernel(k) in looping}


def _frames_for(ns):
    return 1 if ns >= 4096 else 2


def _build_cases():
    cases = []

    def add(group, name, nf=2, recipe="random_target", seed=1234, steps=0, **kw):
        c = Cfg(**kw)
        assert legal(c), (name, illegal_reason(c))
        cases.append(Case(f"{group}-{name}", group, c, nf, recipe, seed + len(cases), steps))

    # -- range stage: every (N, input type), the Q15 window at every N; n_doppler 32
    for ns in N_RANGE:
        for dt in IN_DTYPES:
            add("range", f"{ns}-{dt}", _frames_for(ns), "uniform", n_range=ns, in_dtype=dt)
        add("range", f"{ns}-i16-q15", _frames_for(ns), "uniform", n_range=ns, in_dtype="i16", window="q15_rtl")
    for ns in (4096, 8192):     # several groups per workgroup loop: 3 frames x 2 rx
        add("range", f"{ns}-i16-3fx2rx", 3, "uniform", n_range=ns, n_rx=2, in_dtype="i16")

    # -- whole path, K1: every (N, input type, spectrum) with the fused Doppler weight
    for ns in N_RANGE:
        for dt in IN_DTYPES:
            for sp in SPECTRA:
                add("process", f"k1-{ns}-{dt}-{sp}", _frames_for(ns), "random_target" if sp != "f32" else "two_targets",
                    n_range=ns, n_doppler=64 if sp == "s48" else 32, in_dtype=dt, spectrum=sp, cfar="os1d")
            # the fp16-spectrum K1 without the Doppler weight (MTI on: K2 windows after the canceller)
            add("process", f"k1-{ns}-{dt}-f16-mti2", _frames_for(ns), n_range=ns, in_dtype=dt, spectrum="f16",
                mti=2, cfar="os1d")
        # range_shift log2(N) - 1: the 16-bit spectrum words of the 20000-count target fill int16
        add("process", f"k1-{ns}-i16-q15", _frames_for(ns), n_range=ns, in_dtype="i16", window="q15_rtl",
            range_shift=ns.bit_length() - 2, cfar="os1d")
    for ns in (4096, 8192):
        add("process", f"k1-{ns}-i16-s48-3fx2rx", 3, n_range=ns, n_doppler=64, n_rx=2, in_dtype="i16",
            spectrum="s48", cfar="os1d")

    # -- whole path, K2 on the fp32 and fp16 spectra: FAST, generic (a non-reference 1-D CFAR), MTI
    # 2 / 3, at n_range 64 (T = 16); where the prefetch addressing depends on T, also at the largest
    # T that divides P = NC / 16
    t_fit = {32: 2048, 64: 1024, 128: 256}
    for nc in N_DOPPLER:
        for sp in ("f32", "f16"):
            nrx = 3 if nc == 128 else 2
            add("process", f"k2-{nc}-{sp}-fast-nrx{nrx}", n_doppler=nc, n_rx=nrx, spectrum=sp, cfar="os1d")
            add("process", f"k2-{nc}-{sp}-gen", n_doppler=nc, spectrum=sp, cfar="os1d", cfar1d=(6, 1, 9, 3.0))
            if nc in t_fit:
                add("process", f"k2-{nc}-{sp}-fast-uniform", n_range=t_fit[nc], n_doppler=nc, spectrum=sp, cfar="os1d")
                add("process", f"k2-{nc}-{sp}-gen-uniform", n_range=t_fit[nc], n_doppler=nc, spectrum=sp,
                    cfar="os1d", cfar1d=(6, 1, 9, 3.0))
            if nc == 1024:      # 8-byte points: the XCD remap at T = 2
                add("process", f"k2-{nc}-{sp}-fast-xcd", 1, n_range=2048, n_doppler=nc, spectrum=sp, cfar="os1d")
            # MTI kernels; they also carry the 2-D CFAR cases
            add("process", f"k2-{nc}-{sp}-mti2", n_doppler=nc, n_rx=2 if sp == "f32" else 1, spectrum=sp, mti=2,
                cfar="os2d", compat_cfar=sp == "f16",
                # compat CFAR: the map scaled into the 17-bit word range (noise floor ~2^5, target clipped)
                range_shift=(64 * nc).bit_length() - 8 if sp == "f16" else 0)
            add("process", f"k2-{nc}-{sp}-mti3", n_doppler=nc, spectrum=sp, mti=3,
                cfar="os2d" if sp == "f32" else "os1d", cfar2d=CFAR2D_SETS[1])
    add("process", "k2-256-f32-fast-config2-nrx2", n_range=1024, n_doppler=256, n_rx=2, cfar="os1d")
    add("process", "k2-32-f32-fast-64x32", n_range=64, n_doppler=32, cfar="os1d")   # frame-minor tile order

    # -- whole path, K2 on the S48 spectrum: quad (n_range 64: T = 16), strided quads (1024),
    # pairs (2048); FAST with NCI, generic with the dB map
    for nc in N_DOPPLER[1:]:
        for form, ns in (("quad", 64), ("strided", 1024), ("pair", 2048)):
            nf = 1 if ns * nc >= 1 << 20 else 2
            add("process", f"k2-{nc}-s48-{form}-fast-nrx2", nf, n_range=ns, n_doppler=nc, n_rx=2, spectrum="s48",
                cfar="os1d")
            add("process", f"k2-{nc}-s48-{form}-gen", nf, n_range=ns, n_doppler=nc, spectrum="s48", cfar="os1d",
                cfar1d=(6, 1, 9, 3.0))
    # the quad form with P = NC / 16 lanes per row: P < T (per-point prefetch, exponent exchange
    # inside a 4-lane row) at every such geometry, and P a multiple of T = 8 at NC = 128
    for ns, nc in ((64, 64), (128, 64), (256, 64), (512, 64), (128, 128), (64, 128)):
        add("process", f"k2-{nc}-s48-quad-p<t-{ns}", n_range=ns, n_doppler=nc, spectrum="s48", cfar="os1d")
    add("process", "k2-128-s48-quad-fast-uniform", n_range=256, n_doppler=128, spectrum="s48", cfar="os1d")
    add("process", "k2-128-s48-quad-gen-uniform", n_range=256, n_doppler=128, spectrum="s48", cfar="os1d",
        cfar1d=(6, 1, 9, 3.0))
    add("process", "k2-64-s48-quad-fast-nrx3", n_range=128, n_doppler=64, n_rx=3, spectrum="s48", cfar="os1d")

    # -- whole path, the generic kernel's runtime branches at every Doppler size and on every
    # spectrum form: AMBM (n_range so that n_range * n_doppler >= 2^15: the floor() steps of 1 stay
    # below 1e-5 of the smallest bin check_map looks at), the dB map, the integer Doppler window
    for nc in N_DOPPLER:
        for name, sp, ns in (("f32", "f32", 64), ("f16", "f16", 64), ("s48-quad", "s48", 64),
                             ("s48-strided", "s48", 1024), ("s48-pair", "s48", 2048)):
            if sp == "s48" and nc < 64:
                continue
            nf = 1 if ns * nc >= 1 << 20 else 2
            rec = "two_targets" if sp == "f32" else "random_target"
            ns_ambm = max(ns, min(512, 32768 // nc)) if ns == 64 else ns      # <= 512: still T >= 8
            add("process", f"k2-{nc}-{name}-ambm", nf, rec, n_range=ns_ambm, n_doppler=nc, in_dtype="i16",
                spectrum=sp, magnitude="ambm", cfar="os1d")
            add("process", f"k2-{nc}-{name}-db", nf, rec, n_range=ns, n_doppler=nc, spectrum=sp, map_kind="db",
                cfar="os1d")
        add("process", f"k2-{nc}-q15d", n_doppler=nc, in_dtype="i16", window="q15_rtl", range_shift=5, cfar="os1d")

    # -- 1-D CFAR, stage and fused, n_range 64, 2 frames
    multi = {32: (0, 4.0), 64: (7, 4.0), 128: (11, 4.0), 256: (11, 1.5), 512: (7, 1.5), 1024: (0, 4.0)}
    for nc in N_DOPPLER:
        sets = [(8, 2, 12, 4.0), (8, 2, multi[nc][0], multi[nc][1]), (8, 2, 15, 4.0), (12, 3, 18, 4.0),
                (20, 3, 30, 4.0), (16, 0, 31, 4.0), (6, 1, 9, 3.0)]
        for p in sets:
            kw = dict(n_doppler=nc, window="none", cfar="os1d", cfar1d=p)
            if legal(Cfg(**kw)):        # legal() trims the sets an NC does not allow
                add("cfar1d", f"{nc}-ref{p[0]}-g{p[1]}-rank{p[2]}-a{p[3]}", recipe="map", **kw)
        add("cfar1d", f"{nc}-compat", recipe="map", n_doppler=nc, window="none", cfar="os1d", compat_cfar=True)

    # -- 2-D CFAR stage on crafted maps (cfar2d_map), 3 frames: f = g % nf mixes the frames over the
    # strips, and nf is no multiple of 8.  At the multi-step shape (8 steps per frame) strips of 1, 3
    # (down, up, a short down strip), 5 (down, a short up strip) and the cost model's choice on the
    # reference window (the level screen) and (2, 1, 3, 1) (the generic kernel); every other window
    # once; compat, rank 0 (dense: nearly every tested cell detects) and n_ref - 1, the scale
    # override and two more scale sets on both kernels
    def add2d(name, nc, ns, w, steps, **kw):
        add("cfar2d", f"{nc}x{ns}-w{'.'.join(map(str, w))}-{name}", 3, "map2d", steps=steps, n_range=ns,
            n_doppler=nc, window="none", cfar="os2d", cfar2d=w, **kw)

    for nc in N_DOPPLER:
        ns = cfar2d_shape(nc)
        for w in CFAR2D_SETS[:2]:
            for steps in CFAR2D_STEPS + (0,):
                add2d(f"steps{steps}", nc, ns, w, steps)
        for w in CFAR2D_SETS[2:]:
            if legal(Cfg(n_range=ns, n_doppler=nc, cfar="os2d", cfar2d=w)):
                add2d("steps3", nc, ns, w, 3)
        for w in CFAR2D_SETS[:2]:
            add2d("compat", nc, ns, w, 3, compat_cfar=True)
            add2d("rank0", nc, ns, w, 3, cfar2d_rank_pct=0)
            add2d("rank100", nc, ns, w, 3, cfar2d_rank_pct=100)
            add2d("ovr3", nc, ns, w, 3, cfar2d_override=3)
            add2d("scales222", nc, ns, w, 3, cfar2d_scales=(2, 2, 2))
            add2d("scales135", nc, ns, w, 3, cfar2d_scales=(1, 3, 5))
    # at NC = 1024 compat is a template switch of the reference window's kernel (k_cfar2d_lv CMP)
    add2d("compat-ovr3", 1024, 64, CFAR2D_SETS[0], 3, compat_cfar=True, cfar2d_override=3)
    add2d("compat-rank0", 1024, 64, CFAR2D_SETS[0], 3, compat_cfar=True, cfar2d_rank_pct=0)
    add2d("compat-rank100", 1024, 64, CFAR2D_SETS[0], 3, compat_cfar=True, cfar2d_rank_pct=100)
    for w in CFAR2D_SETS[:2]:       # n_range < TR: half a step (two wave tiles)
        add2d("partial", 32, 64, w, 1)

    # -- whole path, the integer datapath (test_gpu_matrix.test_integer_path): i16 cubes at n_range
    # 64 (T = 16; the MTI kernels have no prefetch and K2's geometry depends on NC only), 2 frames,
    # every Doppler size and both cancellers.  Appended last, with seeds of their own, so the
    # cases above keep theirs.
    def addi(name, nc, m, kind, recipe, nf=2, chunk_frames=0, **kw):
        # "int_clean": the smallest range_shift at which the fp64 oracle clips nowhere (INT_CLEAN_SHIFT,
        # held by test_integer_case_is_not_vacuous); "int_sat": the target's spectrum words just
        # beyond int16 (Hamming: 20000 x 0.54 x 64 / 2^4 = 43 k; Q15, 2x gain less its clipping: / 2^5)
        q15 = kind != "compat"
        shift = INT_CLEAN_SHIFT[nc, m, kind] if recipe == "int_clean" else 5 if q15 else 4
        c = Cfg(n_doppler=nc, in_dtype="i16", window="q15_rtl" if q15 else "hamming", mti=m,
                compat_mti=kind != "q15", range_shift=shift, **kw)
        assert legal(c), (name, illegal_reason(c))
        # "int_clean" seeds are moved on (INT_SEED_MOVED) where synth's random target falls near zero
        # Doppler in a frame: the canceller then leaves that frame's peak at the level where one
        # spectrum word that rounds differently in fp32 and fp64 shows in the frame-level 1e-4
        seed = 7000 + 64 * N_DOPPLER.index(nc) + 8 * m + len(kind)
        if recipe == "int_clean":
            seed += 1000 * INT_SEED_MOVED.get((nc, m, kind), 0)
        cases.append(Case(f"process-int-{nc}-mti{m}-{name}", "process", c, nf, recipe, seed, 0, chunk_frames))

    for nc in N_DOPPLER:
        for m in (2, 3):
            addi("compat", nc, m, "compat", "int_clean", n_rx=3 if nc == 128 else 2, cfar="os2d")
            addi("compat-sat", nc, m, "compat", "int_sat", n_rx=2, cfar="os1d")
            addi("q15", nc, m, "q15", "int_clean", n_rx=1, cfar="os1d")
            addi("q15-sat", nc, m, "q15", "int_sat", n_rx=2, cfar="os2d")
            # the FPGA's own configuration: Q15 windows, word canceller, AMBM, integer CFAR
            addi("chain", nc, m, "chain", "int_clean", n_rx=1, magnitude="ambm", compat_cfar=True,
                 cfar="os1d" if m == 2 else "os2d")
    # the flag adds nothing once the Q15 window is set: test_integer_path also runs this case without it
    addi("q15-compat-same", 128, 2, "chain", "int_sat", n_rx=2, cfar="os1d")
    # the counters over two chunks of one call
    addi("q15-sat-chunked", 64, 3, "q15", "int_sat", nf=3, chunk_frames=2, n_rx=2, cfar="os1d")

    # -- the persistent loops (the section above `loops`): cases of the table above once more under a
    # capped grid, with the fewest frames at which the kernel they are for runs LOOP_MIN iterations in
    # its busiest workgroup, and the largest of the grids 3, 2, 1 (16 for the XCD remap, which is the
    # identity on grids that are no multiple of 8, and on 8) that still does.  Appended last, seeds 9000 and up.
    base = {c.id: c for c in cases}
    n_base = len(cases)

    def loop(base_id, kernel, nf=0, grid=0, name="", **kw):
        b = base[base_id]
        seed = kw.pop("seed", 9000 + len(cases) - n_base + 1000 * LOOP_SEED_MOVED.get(base_id, 0))
        want = ("k2", "xcd") if kernel == "xcd" else (kernel,)
        grids = (grid,) if grid else (16,) if kernel == "xcd" else (3, 2, 1)
        frames = (nf,) if nf else range(b.nf, 65)
        for n in frames:        # the fewest frames first, then the largest grid
            for g in grids:
                c = dataclasses.replace(b, id=f"{b.id}{name}-loop-g{g}", nf=n, grid=g, seed=seed, **kw)
                if set(want) <= set(c.loops()):
                    assert c.cfg.n_range * c.cfg.n_doppler * c.cfg.n_rx * n <= max(MAX_CELLS, b.cfg.n_range * b.cfg.n_doppler * b.cfg.n_rx * b.nf), c.id
                    assert c.id not in base, c.id
                    cases.append(c)
                    base[c.id] = c
                    LOOP_BASE[c.id] = b.id
                    return c
        raise AssertionError((base_id, kernel, "no frame count up to 64 runs the loop"))

    # K1 through fmcw_range_ct: every (N, input type) and the Q15 window
    for ns in N_RANGE:
        for dt in IN_DTYPES:
            loop(f"range-{ns}-{dt}", "k1")
        loop(f"range-{ns}-i16-q15", "k1")
    # K1 through the whole path: the fused Doppler weight on every spectrum (fp16 and S48 stores), the
    # fp16 store without it, the Q15 window (whose saturation count n_sat adds up over the groups)
    for ns in N_RANGE:
        for dt in IN_DTYPES:
            for sp in SPECTRA:
                loop(f"process-k1-{ns}-{dt}-{sp}", "k1")
            loop(f"process-k1-{ns}-{dt}-f16-mti2", "k1")
        loop(f"process-k1-{ns}-i16-q15", "k1")
    # K2: for every K2 key with a twin that is still open, the first whole-path case of the table above
    # that carries it (so every K2 symbol and addressing mode, both tile orders, every NCI and XCD
    # key); then the picks by name below
    open_keys = lambda: {k for k in reachable() if k.endswith("/loop")} - set().union(*(c.keys() for c in cases[n_base:]))  # noqa: E731
    todo = open_keys()
    for b in cases[:n_base]:
        if b.group != "process" or b.recipe in ("int_clean", "int_sat"):
            continue
        mine = {k + "/loop" for k, sym in b.selected() if loopable(k, sym) and loop_kernel(k) in ("k2", "xcd")} & todo
        if mine:
            xcd = any(loop_kernel(k[:-5]) == "xcd" for k in mine)
            # (a case the K1 lines above already run under a grid: once more, with the frames K2 needs)
            todo -= loop(b.id, "xcd" if xcd else "k2", name="-k2" if any(i.startswith(b.id + "-loop-g") for i in base) else "").keys()
    # NCI with an even and an odd n_rx on a prefetching kernel (pf = 16: FAST fp32, NC 64 / 128) and
    # on one without (pf = 0: the generic MTI kernels, integer cases below; FAST at NC 1024)
    for bid in ("process-k2-64-f32-fast-nrx2", "process-k2-128-f32-fast-nrx3", "process-k2-1024-f32-fast-nrx2",
                "process-k2-64-s48-quad-fast-nrx3"):
        if not any(i.startswith(bid + "-loop-g") for i in base):
            loop(bid, "k2")
    # the integer datapath: the counters add up over a workgroup's iterations (K1's n_sat over groups,
    # K2's n_wsat / n_msat over tiles); one saturating Q15 and one saturating compat-MTI case (even and
    # odd n_rx on kernels without a prefetch), and one in chunks of 2 of 4 frames, where every launch
    # loops and the second starts at frame 2 (f0, tile0 non-zero)
    loop("process-int-128-mti3-q15-sat", "k2")
    loop("process-int-128-mti2-compat-sat", "k2")
    # (n_rx 3; with its base's seed: INT_CLEAN_SHIFT is the smallest clean shift of that very cube)
    loop("process-int-128-mti2-compat", "k2", seed=base["process-int-128-mti2-compat"].seed)
    loop("process-int-128-mti3-q15-sat", "k2", nf=4, grid=1, name="-chunked", chunk_frames=2)
    # k_cfar1d at every NC (the reference set; the cube of the same map drives K2 FAST as well)
    for nc in N_DOPPLER:
        loop(f"cfar1d-{nc}-ref8-g2-rank12-a4.0", "cfar1d")
        loop(f"cfar1d-{nc}-compat", "cfar1d")
    # K3 with strips of 3 (per frame: down, up, a short down strip; 3 frames, 9 strips): the generic
    # kernel on (2, 1, 3, 1) under 1 workgroup, the level screen (k_cfar2d_lv at NC 1024) on the
    # reference window under 2, rank 0 (dense: K3b's waves take hundreds of candidates each) under 3,
    # compat (a kernel of its own at NC 1024) under 2; and strips of one step at NC 256 under 2 (grids
    # that do not divide 3 frames: a workgroup's strips change frame)
    for nc in N_DOPPLER:
        ns = cfar2d_shape(nc)
        w0, w1 = (".".join(map(str, w)) for w in CFAR2D_SETS[:2])
        loop(f"cfar2d-{nc}x{ns}-w{w1}-steps3", "k3a", grid=1)
        loop(f"cfar2d-{nc}x{ns}-w{w0}-steps3", "k3a", grid=2)
        loop(f"cfar2d-{nc}x{ns}-w{w0}-rank0", "k3a", grid=3)
        loop(f"cfar2d-{nc}x{ns}-w{w1}-rank0", "k3a", grid=3)
        loop(f"cfar2d-{nc}x{ns}-w{w0}-compat", "k3a", grid=2)
    for w in CFAR2D_SETS[:2]:
        loop(f"cfar2d-256x128-w{'.'.join(map(str, w))}-steps1", "k3a", grid=2)
    return tuple(cases)


# range_shift of the "int_clean" cases, (n_doppler, canceller, kind): the smallest at which nothing
# clips in the fp64 oracle (the word range is then used to a factor of 2: test_integer_case_is_not_vacuous)
INT_SEED_MOVED = {(32, 2, "compat"): 1, (32, 3, "chain"): 1, (128, 3, "compat"): 1, (128, 3, "chain"): 1,
                  (256, 3, "q15"): 2, (256, 3, "chain"): 1, (512, 3, "compat"): 1, (1024, 3, "q15"): 1}
INT_CLEAN_SHIFT = {
    (32, 2, "compat"): 5, (32, 2, "q15"): 7, (32, 2, "chain"): 5, (32, 3, "compat"): 5, (32, 3, "q15"): 7, (32, 3, "chain"): 7,
    (64, 2, "compat"): 4, (64, 2, "q15"): 7, (64, 2, "chain"): 5, (64, 3, "compat"): 6, (64, 3, "q15"): 8, (64, 3, "chain"): 8,
    (128, 2, "compat"): 4, (128, 2, "q15"): 7, (128, 2, "chain"): 6, (128, 3, "compat"): 5, (128, 3, "q15"): 8, (128, 3, "chain"): 7,
    (256, 2, "compat"): 5, (256, 2, "q15"): 7, (256, 2, "chain"): 7, (256, 3, "compat"): 6, (256, 3, "q15"): 8, (256, 3, "chain"): 7,
    (512, 2, "compat"): 5, (512, 2, "q15"): 6, (512, 2, "chain"): 7, (512, 3, "compat"): 6, (512, 3, "q15"): 8, (512, 3, "chain"): 8,
    (1024, 2, "compat"): 5, (1024, 2, "q15"): 7, (1024, 2, "chain"): 7, (1024, 3, "compat"): 5, (1024, 3, "q15"): 8, (1024, 3, "chain"): 7,
}


# capped-grid cases (by their base's id) whose seed is moved on by 1000: fp16 spectrum with MTI on,
# synth's random target near zero Doppler; the canceller removes it, and the format's rounding alone
# (in fp64, no kernel) is then 4.4e-3 of what is left as the frame's peak
# (test_kernel_matrix.test_case_is_fair_to_the_fp16_spectrum)
# Likewise on the fp32 spectrum with the 3-pulse canceller: one frame's target is cancelled to 1 / 70
# .. 1 / 600 of the other frames' peak, and K1's fp32 rounding of the uncancelled spectrum shows in
# that frame's significant bins beyond 1e-4 (the phenomenon of INT_SEED_MOVED;
# test_kernel_matrix.test_mti_case_keeps_every_frames_target).  "process-k2-64-s48-strided-gen": one
# cell of 2 x 1024 x 64 lay 1.04e-4 of its threshold from it in the fp64 map, and the S48 map, itself
# within 1e-4, decided it the other way (check_near_threshold allows 1e-4).  In all of these the
# capped and the uncapped run gave the same bytes.
LOOP_SEED_MOVED = {"process-k1-4096-f16-f16-mti2": 1, "process-k2-32-f32-mti3": 2, "process-k2-256-f32-mti3": 1,
                   "process-k2-512-f32-mti3": 1, "process-k2-64-s48-strided-gen": 1}
LOOP_BASE = {}          # id of a capped-grid case -> id of the case it repeats
CASES = _build_cases()


# ---- inputs and references ----------------------------------------------------------------
def to_complex(cube, dtype):
    if dtype == "f32":
        return cube.astype(np.complex128)
    x = cube.astype(np.float64)
    return x[..., 0] + 1j * x[..., 1]


def make_cube(case: Case):
    """The case's input cube [frame][rx][chirp][sample] in the case's input type."""
    from fmcw import synth
    c = case.cfg
    shape = (case.nf, c.n_rx, c.n_doppler, c.n_range)
    if case.recipe == "uniform":     # white full-scale noise: every range bin is significant
        rng = np.random.default_rng(case.seed)
        if c.in_dtype == "f32":
            return (rng.uniform(-3e4, 3e4, shape) + 1j * rng.uniform(-3e4, 3e4, shape)).astype(np.complex64)
        if c.in_dtype == "i16":
            return rng.integers(-32768, 32768, shape + (2,)).astype(np.int16)
        return rng.uniform(-1, 1, shape + (2,)).astype(np.float16)
    if case.recipe == "int_clean":
        # synth's random target plus noise at half scale (10000 and +-50 counts): the Q15 range
        # window's 2x gain would clip the full-scale target whatever the range_shift
        return synth.frames(case.nf, c.n_range, c.n_doppler, c.n_rx, "random_target", seed=case.seed, dtype="i16") >> 1
    if case.recipe == "int_sat":
        return int_sat_cube(case)
    return synth.frames(case.nf, c.n_range, c.n_doppler, c.n_rx, case.recipe, seed=case.seed, dtype=c.in_dtype)


def int_sat_cube(case: Case):
    """int16 [frame][rx][chirp][sample][2] that clips at every stage of the integer datapath: a
    target of about 20000 counts one Doppler bin below Nyquist (consecutive spectrum words alternate
    in sign, so both cancellers work at their full gain 2 / 4), zero-Doppler clutter of 3000 counts
    in another range bin (the canceller removes it after its first chirps) and uniform noise of +-300
    counts.  Range bins and amplitude differ per frame, and rx r is scaled by 1, 0.6, 0.8: a count
    taken from the wrong frame or rx changes the total."""
    c = case.cfg
    ns, nc = c.n_range, c.n_doppler
    rng = np.random.default_rng(case.seed)
    n = np.arange(ns)[None, :]
    ch = np.arange(nc)[:, None]
    x = np.empty((case.nf, c.n_rx, nc, ns), np.complex128)
    for f in range(case.nf):
        r_t, r_c, a_t = (0.3 + 0.11 * f) * ns + 0.3, (0.77 - 0.05 * f) * ns + 0.6, 20000.0 - 1500.0 * f
        for rx in range(c.n_rx):
            ph = 0.25 * rx
            tone = a_t * np.exp(2j * np.pi * (r_t * n / ns + (nc // 2 - 1) * ch / nc + ph)) \
                + 3000.0 * np.exp(2j * np.pi * (r_c * n / ns + 0.1 + ph))
            x[f, rx] = (1.0, 0.6, 0.8)[rx % 3] * tone + 300.0 * (rng.uniform(-1, 1, (nc, ns)) + 1j * rng.uniform(-1, 1, (nc, ns)))
    iq = np.stack([np.rint(x.real), np.rint(x.imag)], axis=-1)
    return np.clip(iq, -32768, 32767).astype(np.int16)


# ---- the integer datapath's references (cases "process-int-*") ------------------------------
def int_spectrum(case: Case, cube):
    """The fp64 oracle's scaled range spectrum [frame][rx][range][chirp] of an integer-path case."""
    import fmcw_oracle as O
    c = case.cfg
    if c.window == "q15_rtl":
        spec = O.range_ct(O.window_q15_cube(cube), window=False)
    else:
        spec = O.range_ct(to_complex(cube, "i16"))
    return spec * 2.0 ** -c.range_shift


def int_counts(c: Cfg, cube, spec):
    """fmcw_oracle.WordClips of a scaled range spectrum [frame][rx][range][chirp] (the oracle's or the
    GPU's own) and, with the Q15 window, of the cube in the range window: summed over frames and rx."""
    import fmcw_oracle as O
    q15 = c.window == "q15_rtl"
    n = O.word_clips(np.asarray(spec).astype(np.complex128), c.mti, q15)
    return n._replace(range_window=O.range_window_clips(cube) if q15 else 0)


def ambm_f64(rd):
    """magnitude_calc.vhd:57-81 on an fp64 spectrum."""
    ai, aq = np.abs(rd.real), np.abs(rd.imag)
    mx, mn = np.maximum(ai, aq), np.minimum(ai, aq)
    return mx + np.floor(mn / 4) + np.floor(mn / 8)


def int_map(c: Cfg, spec):
    """The oracle's map [frame][range][doppler] (fp64) from a scaled range spectrum [frame][rx][range]
    [chirp]: the Doppler stage in RTL arithmetic (16-bit words, saturating canceller, the Hamming or
    the integer Q15 window), then NCI over rx or AMBM."""
    import fmcw_oracle as O
    q15 = c.window == "q15_rtl"
    out = []
    for f in range(spec.shape[0]):
        rd = O.doppler_stage(np.asarray(spec[f]).astype(np.complex128), window=not q15, mti_mode=c.mti,
                             q15_rtl=q15, mti_rtl=True)
        out.append(ambm_f64(rd[0]) if c.magnitude == "ambm" else O.magnitude(rd, rx_axis=0))
    return np.stack(out)


def cfar1d_map(case: Case):
    """[frame][range][doppler] float32 map for a 1-D CFAR case: integer-valued Rayleigh clutter,
    spikes at the corners of the map and of the 16-cell lane blocks, and a constant patch whose
    centre cell equals alpha x the patch value (cut == threshold: a tie, not a detection)."""
    c = case.cfg
    ns, nc = c.n_range, c.n_doppler
    ref, guard, rank, alpha = c.cfar1d
    rng = np.random.default_rng(case.seed)
    m = np.floor(rng.rayleigh(12.0, (case.nf, ns, nc))).astype(np.float32)
    big = 60000.0 if c.compat_cfar else 1.0e6
    for f in range(case.nf):
        # one spike per row: no spike is a reference cell of another, whatever the window
        for r, d in ((0, 0), (1, 16 % nc), (ns - 1, nc - 1), (2, 15), (ns // 2, nc // 2), (3, nc - 1),
                     (ns - 2, 0), (7, 31 % nc), (9, (nc - 16) % nc)):
            m[f, r, d] = big + 16 * r + d
    h = ref + guard
    # the patch: every reference cell of its centre holds 8, the centre alpha * 8 (an integer)
    for f, r, dc in ((0, 20, nc // 4), (case.nf - 1, 41, 0)):
        for o in range(-h, h + 1):
            m[f, r, (dc + o) % nc] = 8.0
        m[f, r, dc % nc] = np.float32(alpha) * np.float32(8.0)
    # cells that decide at the edge of the group screen: the cut equals its 4 nearest right
    # references (row 30) or its whole right side (row 33), every other window cell is 1, so exactly
    # 4 / ref references reach cut / alpha, in whole groups of 4 -- a detection iff that count is
    # below n_ref - rank, which a screen that is off by one group gets wrong
    for r, n_high in ((30, 4), (33, ref)):
        dc = nc // 2 + 3
        for o in range(-h, h + 1):
            m[0, r, (dc + o) % nc] = 1.0
        for j in range(min(n_high, ref)):
            m[0, r, (dc + guard + 1 + j) % nc] = 4096.0
        m[0, r, dc] = 4096.0
    return m


def cube_from_map(m):
    """A cube (window "none", one rx) whose range-Doppler magnitude is the map, up to fp32 rounding."""
    x = np.fft.ifft2(m.astype(np.float64), axes=(-2, -1))       # [frame][sample][chirp]
    return np.ascontiguousarray(np.swapaxes(x, -1, -2)[:, None]).astype(np.complex64)


def cfar1d_oracle(m, c: Cfg):
    """(detections O.DET_DTYPE, det masks, thresholds) of the oracle 1-D CFAR on float32 maps."""
    import fmcw_oracle as O
    p = O.Cfar1D(*c.cfar1d[:3], alpha=c.cfar1d[3])
    dets, masks, thrs = [], [], []
    for f in range(m.shape[0]):
        if c.compat_cfar:
            det, thr = O.cfar_os1d_rtl(m[f], p)
            dets.append(O.detections_rtl(det, m[f], thr, frame=f))
        else:
            det, thr = O.cfar_os1d(m[f], p)
            dets.append(O.detections(det, m[f], thr, frame=f))
        masks.append(det)
        thrs.append(thr)
    return np.concatenate(dets), np.stack(masks), np.stack(thrs)


def cfar2d_offsets(c: Cfg):
    """The reference cells (dr, dd) of a CUT in the fixed order (fmcw_oracle.cfar2d_offsets)."""
    hr, gr, hd, gd, _, _ = cfar2d_geom(c)
    return [(dr, dd) for dr in range(-hr, hr + 1) for dd in range(-hd, hd + 1)
            if not (abs(dr) <= gr and abs(dd) <= gd)]


def cfar2d_spike_rows(case: Case):
    """(tested, untested) range rows that carry a spike: the first and last tested rows hr and
    ns - hr - 1, the untested rows next to them, and the two rows either side of every step
    boundary k TR (every strip boundary is one)."""
    c = case.cfg
    ns, tr, hr = c.n_range, cfar2d_TR(c.n_doppler), cfar2d_geom(c)[0]
    rows = {hr, ns - hr - 1}
    if hr:
        rows |= {hr - 1, ns - hr}
    for k in range(1, -(-ns // tr)):
        rows |= {k * tr - 1, k * tr}
    tested = sorted(r for r in rows if hr <= r < ns - hr)
    return tested, sorted(rows - set(tested))


def cfar2d_scales_reachable(c: Cfg):
    """The scales the bracket (os_cfar_2d.vhd:189-213) can choose: ranked > 1.5 mean needs a
    reference below the ranked one (rank > 0), ranked < mean / 2 one above it (rank < n_ref - 1)."""
    _, _, _, _, n_ref, rank = cfar2d_geom(c)
    smin, snom, smax = c.cfar2d_scales
    return ([smin] if rank <= n_ref - 2 else []) + [snom] + ([smax] if rank >= 1 else [])


@functools.lru_cache(maxsize=4)
def cfar2d_layout(case: Case):
    """(maps [frame][range][doppler] float32, marks {name: (frame, range, doppler)}) of a 2-D CFAR
    case, deterministic from its seed.

    Rayleigh clutter (sigma 12; integer-valued for compat) with a bright patch (sigma 150) and a
    quiet patch; a 1e30 cell, a negative cell and a -0.0 (fmcw_cfar takes both as +0).  Spikes, one per
    row and frame so that none is a reference cell of another under the windows whose rank is
    n_ref - 1 (hd <= 6): in tested row j of cfar2d_spike_rows at Doppler 16 j (frame 0: cells 0 and
    16), NC - 1 - 16 j (frame 1) and 16 j + 15 (frame 2), all mod NC; in the untested rows at
    NC / 2 + 8.  Then window-sized blocks whose centre CUT has every reference cell set by hand:
      tie / nom_det    all references 8: mean 8, ranked 8, the nominal scale (or the override) S;
                       centre S x 8 (cut == threshold: no detection) and S x 8 + 1
      max_tie / _det   n_ref - rank references 64, the rest 1: ranked 64 > 1.5 mean, scale_max
      min_tie / _det   one reference 4096, the rest 1: ranked 1 < mean / 2, scale_min
      zero_det / zero_cut0   a block of +0 one cell wider than the window: the centre 1.0 detects
                       (threshold 0), the +0 cell next to it does not
      denorm_det       the same with a few 1e-40 references and the centre 1e-39 (not compat)
    The scale blocks lie in frame 0, the zero blocks in frame 1."""
    c = case.cfg
    ns, nc, nf = c.n_range, c.n_doppler, case.nf
    hr, gr, hd, gd, n_ref, rank = cfar2d_geom(c)
    smin, snom, smax = c.cfar2d_scales
    compat = c.compat_cfar
    rng = np.random.default_rng(case.seed)
    quant = np.floor if compat else (lambda x: x)
    m = quant(rng.rayleigh(12.0, (nf, ns, nc))).astype(np.float32)
    # the patches of test_gpu_r05_k3._clutter, scaled to the shape
    r0, d0, pr, pd = 3 * ns // 8, nc // 5, max(ns // 12, 2 * hr + 3), max(nc // 16, 4)
    m[:, r0:r0 + pr, d0:d0 + pd] = quant(rng.rayleigh(150.0, (nf, pr, pd)))
    r0, d0, pr, pd = 11 * ns // 16, 5 * nc // 8, max(ns // 8, 2 * hr + 3), max(nc // 10, 4)
    m[:, r0:r0 + pr, d0:d0 + pd] = 1.0 if compat else 0.02
    r_odd = min(max(ns // 4 + 2, hr), ns - hr - 1)
    if not compat:
        m[2, r_odd, (nc // 2 + 8) % nc] = 1e30            # far above every key window (frame 2: no blocks)
    m[2, r_odd, 8] = -5.0
    m[2, r_odd, 10] = -0.0
    marks = {}
    tested, untested = cfar2d_spike_rows(case)
    spike = (lambda r, d: 50000.0 + (16 * r + d) % 8192) if compat else (lambda r, d: 1.0e6 + 16 * r + d)
    for j, r in enumerate(tested):
        for f, d in enumerate((16 * j % nc, (nc - 1 - 16 * j) % nc, (16 * j + 15) % nc)):
            m[f, r, d] = spike(r, d)
    for r in untested:
        m[:, r, (nc // 2 + 8) % nc] = spike(r, nc // 2 + 8)

    # ---- the blocks: centres on a grid of (2 hr + 3) x (2 hd + 3) cells below the first tested row
    band, wd = 2 * hr + 3, 2 * hd + 3
    per = max(1, nc // wd)

    def centres(n):
        nb = -(-n // per)
        first, last = 3 * hr + 3, ns - hr - 2
        if len(tested) > 1 and tested[1] + hr + 2 + (nb - 1) * band <= last:
            first = max(first, tested[1] + hr + 2)    # below the second tested spike row too (Doppler 16)
        stride = max(band, (last - first) // nb) if nb > 1 else band
        assert first + (nb - 1) * stride <= last, (case.id, "no room for the blocks")
        return [(first + (i // per) * stride, (hd + 1 + (i % per) * wd) % nc) for i in range(n)]

    offs = cfar2d_offsets(c)

    def block(f, name, rd, refs, centre):
        r, d = rd
        for (dr, dd), v in zip(offs, refs):
            m[f, r + dr, (d + dd) % nc] = v
        m[f, r, d] = centre
        marks[name] = (f, r, d)

    s_eff = c.cfar2d_override or snom
    todo = [("tie", [8.0] * n_ref, s_eff * 8.0), ("nom_det", [8.0] * n_ref, s_eff * 8.0 + 1)]
    if not c.cfar2d_override:
        if rank >= 1:                                  # cfar2d_scales_reachable
            refs = [64.0] * (n_ref - rank) + [1.0] * rank
            assert 64.0 > 1.5 * sum(refs) / n_ref + 1
            todo += [("max_tie", refs, smax * 64.0), ("max_det", refs, smax * 64.0 + 1)]
        if rank <= n_ref - 2:
            refs = [4096.0] + [1.0] * (n_ref - 1)
            todo += [("min_tie", refs, smin * 1.0), ("min_det", refs, smin * 1.0 + 1)]
    for (name, refs, centre), rd in zip(todo, centres(len(todo))):
        block(0, name, rd, refs, centre)
    zeros = ["zero_det"] + ([] if compat else ["denorm_det"])
    for name, (r, d) in zip(zeros, centres(len(zeros))):
        for dd in range(-hd - 1, hd + 2):
            m[1, r - hr - 1:r + hr + 2, (d + dd) % nc] = 0.0
        if name == "zero_det":
            m[1, r, d] = 1.0
            marks[name] = (1, r, d)
            marks["zero_cut0"] = (1, r, (d + 1) % nc) if hd else (1, r + 1, d)
        else:
            n_d = min(3, n_ref - rank - 1)            # the ranked reference stays +0
            block(1, name, (r, d), [1e-40] * n_d + [0.0] * (n_ref - n_d), 1e-39)
    m.setflags(write=False)
    return m, marks


def cfar2d_source_constants():
    """(kCoopRound, the detection slot's floor and divisor with det_capacity set) read from the
    sources: cfar2d.hpp `kCoopRound`, plan.hip build_plan's `slot_cap` (max(floor, cells per tile / divisor))."""
    import re
    from pathlib import Path
    src = Path(__file__).resolve().parent.parent / "fpga-fmcw-radar-processor_amd" / "csrc"
    coop = re.search(r"constexpr int kCoopRound = (\d+);", (src / "cfar2d.hpp").read_text())
    slot = re.search(r"p\.slot_cap = \(uint32_t\)\(c\.det_capacity \? std::max<size_t>\((\d+), cells_tile / (\d+)\) : cells_tile\);",
                     (src / "plan.hip").read_text())
    assert coop and slot, "kCoopRound / slot_cap are no longer where the matrix reads them"
    return int(coop.group(1)), int(slot.group(1)), int(slot.group(2))


def cfar2d_dense(c: Cfg) -> bool:
    """rank 0: the threshold is scale x the smallest reference, nearly every tested cell detects.
    These cases run with det_capacity set (test_gpu_matrix), where a wave tile's slot holds 1/32 of
    its cells and denser tiles move to the sink's overflow region (det_sink.hpp det_reserve_wave);
    with det_capacity 0, as every other case runs, a slot holds the whole tile."""
    return c.cfar == "os2d" and cfar2d_geom(c)[5] == 0


def cfar2d_map(case: Case):
    """The [frame][range][doppler] float32 maps of a 2-D CFAR case (cfar2d_layout)."""
    return cfar2d_layout(case)[0]


def cfar2d_clamped(m):
    """fmcw_cfar takes negative cells and -0.0 as +0 (det_sink.hpp nonneg); the references see that map."""
    return np.where(m > 0, m, np.float32(0.0)).astype(np.float32)


def cfar2d_oracle(m, c: Cfg, frames=None):
    """(detections O.DET_DTYPE, det masks, thresholds) of the NumPy oracle 2-D CFAR (RTL integers
    for compat) on the clamped maps; `frames`: only these frames."""
    import fmcw_oracle as O
    p = oracle_cfar(c)
    mc = cfar2d_clamped(m)
    dets, masks, thrs = [], [], []
    for f in (range(m.shape[0]) if frames is None else frames):
        if c.compat_cfar:
            det, thr = O.cfar_os2d_rtl(mc[f], p)
            dets.append(O.detections_rtl(det, mc[f], thr, frame=f))
        else:
            det, thr = O.cfar_os2d(mc[f], p)
            dets.append(O.detections(det, mc[f], thr, frame=f))
        masks.append(det)
        thrs.append(thr)
    return np.concatenate(dets), np.stack(masks), np.stack(thrs)


def oracle_cfar(c: Cfg):
    import fmcw_oracle as O
    if c.cfar == "os1d":
        return O.Cfar1D(*c.cfar1d[:3], alpha=c.cfar1d[3])
    rr, gr, rd, gd = c.cfar2d
    smin, snom, smax = c.cfar2d_scales
    return O.Cfar2D(ref_range=rr, guard_range=gr, ref_doppler=rd, guard_doppler=gd, rank_pct=c.cfar2d_rank_pct,
                    scale_min=smin, scale_nom=snom, scale_max=smax, scale_override=c.cfar2d_override)


def oracle_dets(maps, c: Cfg):
    """The oracle CFAR of the configuration on float32 maps [frame][range][doppler]."""
    import fmcw_oracle as O
    p = oracle_cfar(c)
    out = []
    for f in range(maps.shape[0]):
        if c.compat_cfar:
            det, thr = (O.cfar_os1d_rtl if c.cfar == "os1d" else O.cfar_os2d_rtl)(maps[f], p)
            out.append(O.detections_rtl(det, maps[f], thr, frame=f))
        else:
            det, thr = (O.cfar_os1d if c.cfar == "os1d" else O.cfar_os2d)(maps[f], p)
            out.append(O.detections(det, maps[f], thr, frame=f))
    return np.concatenate(out)


@functools.lru_cache(maxsize=2)
def _reference(n_range, n_doppler, n_rx, in_dtype, mti, magnitude, nf, recipe, seed):
    import fmcw_oracle as O
    case = Case("ref", "process", Cfg(n_range, n_doppler, n_rx, in_dtype), nf, recipe, seed)
    cube = make_cube(case)
    ref = []
    for f in range(nf):
        o = O.process(to_complex(cube[f], in_dtype), None, mti_mode=mti)
        if magnitude == "ambm":      # magnitude_calc.vhd:57-81 on the fp64 spectrum
            rd = o["rd"][0]
            ai, aq = np.abs(rd.real), np.abs(rd.imag)
            mx, mn = np.maximum(ai, aq), np.minimum(ai, aq)
            ref.append(mx + np.floor(mn / 4) + np.floor(mn / 8))
        else:
            ref.append(o["mag"])
    ref = np.stack(ref)
    ref.setflags(write=False)
    cube.setflags(write=False)
    return cube, ref


def reference(case: Case):
    """(input cube, fp64 oracle map [frame][range][doppler]) of a whole-path case with an fp32
    window; computed once per input and shared, read-only."""
    c = case.cfg
    assert c.window != "q15_rtl"
    cube, ref = _reference(c.n_range, c.n_doppler, c.n_rx, c.in_dtype, c.mti, c.magnitude, case.nf, case.recipe,
                           case.seed)
    # range_shift scales the fp32 range window by 2^-shift (fmcw_api.hip window_table): exact
    return cube, (ref * 2.0 ** -c.range_shift if c.range_shift else ref)


U16 = 2.0 ** -11          # unit roundoff of fp16 (round to nearest, 11 significant bits)
SUB16 = 2.0 ** -25        # half the spacing of fp16 subnormals: the absolute rounding error below 2^-14


def fp16_row_error(case: Case):
    """E[frame][range]: how far the fp16 spectrum (fmcw.h FMCW_SPEC_F16: half2(X / N_range) between
    K1 and K2, spectrum.hpp pack_h2 rounds to nearest) can move any cell of a range row of the map, from
    the format alone.  A stored point p has |dp| <= U16 |p| + sqrt(2) SUB16 (relative rounding, or
    the subnormal spacing); the canceller sums 2 (4) points' errors; the Doppler FFT output of the
    row moves by at most sum_c w[c] |d[c]|; |.| is 1-Lipschitz, NCI takes the 2-norm over rx, and
    AMBM (mx + floor(mn / 4) + floor(mn / 8)) moves by at most 1.375 times as much plus 2 floor steps."""
    import fmcw_oracle as O
    c = case.cfg
    cube, _ = reference(case)
    w = O.window_f32(c.n_doppler).astype(np.float64)
    out = []
    for f in range(case.nf):
        x = np.abs(O.range_ct(to_complex(cube[f], c.in_dtype))) * 2.0 ** -c.range_shift     # [rx][range][chirp]
        e = U16 * x                                   # relative part, per stored point
        gain = 1.0                                    # the canceller's gain on the absolute part
        if c.mti:
            e1 = np.zeros_like(e)
            e1[..., 1:] = e[..., :-1]
            if c.mti == 2:
                e, gain = e + e1, 2.0
            else:
                e2 = np.zeros_like(e)
                e2[..., 2:] = e[..., :-2]
                e, gain = e + 2 * e1 + e2, 4.0
        # (the absolute part is not weighted: with MTI off K1 stores the point already windowed)
        per_rx = (e * w).sum(axis=-1) + gain * np.sqrt(2.0) * SUB16 * c.n_range * c.n_doppler
        row = np.sqrt((per_rx ** 2).sum(axis=0))                                           # [range]
        out.append(1.375 * row + 2.0 if c.magnitude == "ambm" else row)
    return np.stack(out)


def check_near_threshold(got_dets, ref_mag, c: Cfg, case: Case = None):
    """tests/test_gpu_parity.py::test_process_parity's rule: against the CFAR of the fp64
    end-to-end map, detection lists differ only at cells with |cut - thr| <= 1e-4 thr.

    On the fp16 spectrum that rule cannot hold: the format's rounding moves a cell by up to
    fp16_row_error(), which in a row that holds a target is many times the noise cells' own size.
    There (pass `case`) the 1-D decision may also differ where the cut and the threshold's reference
    cell, both of the cut's row, can have moved that far: |cut - thr| <= 1e-4 thr + (1 + alpha) E[row].
    Returns (differing cells, worst |cut - thr| / thr among them, worst |cut - thr| / margin)."""
    import fmcw_oracle as O
    p = oracle_cfar(c)
    fn = O.cfar_os1d if c.cfar == "os1d" else O.cfar_os2d
    ref32 = ref_mag.astype(np.float32)
    a = set(zip(got_dets["frame"].tolist(), got_dets["range"].tolist(), got_dets["doppler"].tolist()))
    b = set()
    thr = []
    for f in range(ref32.shape[0]):
        det, t = fn(ref32[f], p)
        thr.append(t)
        r, d = np.nonzero(det)
        b |= set(zip([f] * len(r), r.tolist(), d.tolist()))
    E = None
    if c.spectrum == "f16" and case is not None:
        assert c.cfar == "os1d"
        E = fp16_row_error(case)
    worst_rel = worst = 0.0
    bad = []
    for (f, r, d) in sorted(a ^ b):
        gap = abs(ref_mag[f, r, d] - thr[f][r, d])
        margin = 1e-4 * max(thr[f][r, d], 1e-30)
        worst_rel = max(worst_rel, gap / max(thr[f][r, d], 1e-30))
        if E is not None:
            margin += (1 + c.cfar1d[3]) * E[f, r]
        worst = max(worst, gap / margin)
        if gap > margin:
            bad.append((f, r, d, float(gap / margin)))
    assert not bad, f"{len(bad)} decisions differ beyond the margin (frame, range, doppler, gap / margin): {bad[:8]}"
    return len(a ^ b), worst_rel, worst


def check_case_map(c: Cfg, got, ref):
    """The map rule of a whole-path case: check_map (1e-4 per frame and per significant bin) on
    the fp32 and S48 spectra, the stated 2e-3 per frame on the fp16 spectrum."""
    from conftest import rel_err
    from gpu_support import check_map
    if c.spectrum == "f16":
        for f in range(ref.shape[0]):
            e = rel_err(got[f], ref[f])
            assert e <= 2e-3, f"frame {f}: max rel err {e:.3g}"
    else:
        check_map(got, ref)


# ---- the white scene: every cell of the K1 -> K2 map checked -----------------------------------
# check_map holds the map to 1e-4 of the frame's peak, and per bin only above 1e-3 of that peak; on
# `random_target` / `two_targets` (one or two tones over weak noise) that leaves nearly every cell
# outside the targets' rows unchecked (test_kernel_matrix.test_tone_scene_leaves_most_cells_unchecked).
# The cases "<base id>-white" run the configuration, frames, grid and chunking of a case above on
# recipe "uniform" (make_cube: white full-scale noise), where every range row of the map is at full
# scale, under check_every_cell: 1e-4 of the rms of the cell's own range row.
WHITE_TOL = 1e-4          # gpu_support.MAP_TOL, applied to the row's scale instead of the frame's peak
WHITE_SEED = 20000
WHITE_CAP = 0.02          # the largest share of cells in which a wrong map may pass: fp32 and S48 spectrum
WHITE_CAP_F16 = 0.25      # fp16 spectrum, whose rule carries the format's worst-case bound


def _white_admissible(case: Case) -> bool:
    """Whole-path cases that can have a white twin: not the Q15 window, not the integer datapath (its
    references are built on the GPU's own spectrum, and a full-scale input would clip everywhere)."""
    return (case.group == "process" and case.cfg.window != "q15_rtl"
            and case.recipe not in ("int_clean", "int_sat"))


def _white_cfg(case: Case) -> Cfg:
    """A dB case runs with the linear map: the dB map as such is test_whole_path's."""
    return dataclasses.replace(case.cfg, map_kind="linear") if case.cfg.map_kind == "db" else case.cfg


def white_wanted(key: str) -> bool:
    """K1 / K2 keys that loopable() accepts, and their "/loop" twins; and the generic K2's AMBM branch,
    which has no twin but computes another map (check_every_cell has a rule of its own for it)."""
    base = key[:-5] if key.endswith("/loop") else key
    table = reachable_with_symbols()
    if base not in table or not base.startswith(("k_range", "k_doppler")):
        return False
    return loopable(base, table[base]) or key.endswith("/ambm")


def white_targets() -> set:
    """The keys a white twin can exist for: every wanted key of reachable() that some admissible
    whole-path case of CASES claims (a dB case with its linear map)."""
    claimed = set()
    for b in CASES:
        if _white_admissible(b):
            claimed |= dataclasses.replace(b, cfg=_white_cfg(b)).keys()
    return {k for k in reachable() if white_wanted(k)} & claimed


def _build_white():
    todo = white_targets()
    out = []
    for linear_first in (True, False):      # a dB case only for what no linear case claims
        for b in CASES:
            if not _white_admissible(b) or (b.cfg.map_kind == "db") == linear_first:
                continue
            w = dataclasses.replace(b, id=b.id + "-white", cfg=_white_cfg(b), recipe="uniform",
                                    seed=WHITE_SEED + len(out))
            mine = w.keys() & todo
            if mine:
                todo -= mine
                out.append(w)
                WHITE_BASE[w.id] = b.id
    assert not todo, sorted(todo)
    return tuple(out)


WHITE_BASE = {}         # id of a white case -> id of the case whose configuration it runs
WHITE = _build_white()


def row_rms(ref):
    """R[frame][range] = sqrt(mean_d ref[frame][range][d]^2)."""
    return np.sqrt(np.mean(np.square(ref, dtype=np.float64), axis=-1))


def every_cell_bound(c: Cfg, ref, case: Case):
    """[frame][range]: how far a cell of that range row may lie from the fp64 oracle's.  1e-4 of the
    row's rms; on the fp16 spectrum plus the format's bound fp16_row_error (which holds AMBM's two
    floor steps already); AMBM on the other spectra plus those 2 steps, as test_integer_path adds them."""
    bound = WHITE_TOL * row_rms(ref)
    if c.spectrum == "f16":
        bound = bound + fp16_row_error(case)
    elif c.magnitude == "ambm":
        bound = bound + 2.0
    return bound


def check_every_cell(c: Cfg, got, ref, case: Case):
    """The map rule of a white case: every cell of `got` (finite float32 [frame][range][doppler]) within
    every_cell_bound of `ref`, the fp64 oracle map of reference(case).  `c` is the configuration whose rule
    applies (the case's own, or its fp32-spectrum form for an fp32 restatement).  Prints and returns the
    worst fraction of the bound used."""
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == ref.shape, f"{case.id}: got {got.dtype} {got.shape}, reference {ref.shape}"
    assert np.isfinite(got).all(), f"{case.id}: {int((~np.isfinite(got)).sum())} cells are not finite"
    used = np.abs(got.astype(np.float64) - ref) / every_cell_bound(c, ref, case)[..., None]
    worst = float(used.max())
    print(f"{case.id}: worst fraction of the every-cell bound used {worst:.3g}")
    if worst > 1.0:
        f, r, d = np.unravel_index(int(used.argmax()), used.shape)
        raise AssertionError(f"{case.id}: {int((used > 1.0).sum())} of {used.size} cells beyond the bound, the worst at frame {f} "
                             f"range {r} doppler {d}: got {got[f, r, d]:.9g}, reference {ref[f, r, d]:.9g}, "
                             f"{worst:.3g} of the bound")
    return worst


def unchecked_shares_map(ref, bound):
    """The share of cells in which another map passes the every-cell rule (`bound` [frame][range]) against
    `ref` [frame][range][doppler]: zeros, the reference rolled by one range row, by one Doppler bin, and the
    previous frame's map (1.0 by construction where there is one frame)."""
    def share(other):
        return float((np.abs(other - ref) <= bound[..., None]).mean())
    return {"zero": share(np.zeros_like(ref)), "row": share(np.roll(ref, 1, axis=1)),
            "bin": share(np.roll(ref, 1, axis=2)),
            "frame": share(np.roll(ref, 1, axis=0)) if ref.shape[0] > 1 else 1.0}


def unchecked_shares_check_map(ref, fp16=False):
    """The same four shares under the rule of the tone cases (check_case_map): a cell passes where the
    other map is within 1e-4 (fp16 spectrum: 2e-3) of the frame's peak and, on the fp32 and S48 spectra,
    within 1e-4 of the cell itself if the cell is above 1e-3 of that peak."""
    peak = np.abs(ref).max(axis=(1, 2), keepdims=True)

    def share(other):
        err = np.abs(other - ref)
        if fp16:
            return float((err <= 2e-3 * peak).mean())
        return float(((err <= WHITE_TOL * peak) & ((np.abs(ref) < 1e-3 * peak) | (err <= WHITE_TOL * np.abs(ref)))).mean())
    return {"zero": share(np.zeros_like(ref)), "row": share(np.roll(ref, 1, axis=1)),
            "bin": share(np.roll(ref, 1, axis=2)),
            "frame": share(np.roll(ref, 1, axis=0)) if ref.shape[0] > 1 else 1.0}
