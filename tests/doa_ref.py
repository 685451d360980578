"""The angle resolver's specification (include/fmcw.h, "Angle resolution") in fp64 NumPy, and the derived
tolerances the GPU tests hold fmcw_doa_enqueue to.

    w[g]   = fp32(1 / sum_k |A[g][k]|^2)
    y[g]   = sum_k conj(A[g][k]) r[k];   B[g] = |y[g]|^2 w[g];   g* = the lowest g at the largest B
    a      = y[g*] w[g*];                r <- r - a A[g*][:]
    k_max stages (ended by B[g*] == 0, or after the first by B[g*] < min_rel B_0[g_0]), then relax_passes
    passes that put each source back, scan again and cancel again;  pos = g* + parabola offset.

An argmax can legitimately differ between fp32 and fp64 at a near tie, so resolve() takes forced picks: the
GPU's grid points after the stages and after every pass (the runs with relax_passes = 0, 1, ..: a run with
p passes does the arithmetic of one with p + 1 up to its end).  resolve() accepts a pick where it could
have been the maximum within the bound, goes on along it, and bounds everything else.

Tolerances, u = 2^-24, gamma(n) = n u / (1 - n u).  The resolver carries e_r[k], a bound on the distance
between the GPU's residual and this one, from scan to scan (0 at the start: the snapshot is fp32 data):
    y       each component is a chain of 2 n_ch fmas over products whose moduli sum to at most
            S[g] = sum_k |A[g][k]| (|r[k]| + e_r[k]): 2 n_ch roundings per term, both components:
            e_y[g] = sqrt(2) gamma(2 n_ch) S[g] + sum_k |A[g][k]| e_r[k]
    B       e_B[g] = w (2 |y| e_y + e_y^2) + gamma(3) w (|y| + e_y)^2        (a square, an fma, times w)
    a       e_a = w e_y[g*] + u |a|                                          (one product per component)
    r       e_r[k] = e_rho[k] + sum over the sources cancelled at the moment of e_a_j |A[g_j][k]|: each side
            subtracts, and later adds back, its own a_j A[g_j], so that a source's share of the distance
            goes as it came; what stays is the rounding.  r -+ a A is two fmas per component on values up
            to |r[k]| + |a| |A[g*][k]|:  e_rho[k] <- e_rho[k] + 2 sqrt(2) u (|r[k]| + e_r[k] + (|a| + e_a) |A[g*][k]|)
    total, residual   a square, an fma and the 6 adds of the wave's tree on non-negative terms: gamma(8)
            of the sum; the residual also moves by sum_k 2 |r[k]| e_r[k] + e_r[k]^2
    pos     num = B[g-1] - B[g+1], den = B[g-1] - 2 B[g] + B[g+1] move by at most
            E_num = e_B[g-1] + e_B[g+1] + u |num|,  E_den = e_B[g-1] + 2 e_B[g] + e_B[g+1] + 2 u (|B[g-1]| + 2 |B[g]| + |B[g+1]|);
            a source with E_den / |den| >= 0.05 is ill-conditioned and skipped for pos only, at most 5 % of
            a list (tests/test_doa_host.py establishes that on the reference alone); otherwise
            e_pos = (0.5 E_num + |off| E_den) / (|den| - E_den) + 2 u max(g, 1)
    a pick g is accepted where B[g] >= max B - 2 max(e_B[g], e_B[g_ref]); the GPU's n_src where the end
    tests could have gone its way within e_B.
    frame, range, doppler, flags, n_src slots beyond n_src: exact.
"""
import numpy as np

U = 2.0 ** -24
FLAG_NO_SNAPSHOT, FLAG_ONE_CH = 1, 2
COND_MAX = 0.05
SKIP_SHARE = 0.05
DEFECTS = ("unconjugated", "no_w", "no_subtraction", "highest_tie", "parabola_sign", "transposed")


def gamma(n):
    return n * U / (1.0 - n * U)


def weights(steering):
    """w[g] as the library stores it: fp64 sum, fp32 value (0 for a row of norm 0 or not finite)."""
    a = np.asarray(steering, np.complex64).astype(np.complex128)
    with np.errstate(over="ignore", invalid="ignore"):
        norm = (a.real ** 2 + a.imag ** 2).sum(axis=1)
    ok = (norm > 0) & np.isfinite(norm)
    return np.where(ok, 1.0 / np.where(ok, norm, 1.0), 0.0).astype(np.float32).astype(np.float64), ok


class Table:
    """A steering table as the scans read it: A [g][k] complex128 (bad rows zeroed), |A|, w."""

    def __init__(self, steering, defect=None):
        a = np.asarray(steering, np.complex64)
        if defect == "transposed":
            a = a.reshape(-1).reshape(a.shape[1], a.shape[0]).T
        self.w, ok = weights(a)
        self.a = np.where(ok[:, None], a.astype(np.complex128), 0.0)
        self.abs = np.abs(self.a)
        self.n_grid, self.n_ch = self.a.shape
        self.defect = defect
        if defect == "no_w":
            self.w = ok.astype(np.float64)


def _parabola(b, g, refine, sign=1.0):
    """(off, den, num) of the three-point parabola at g."""
    if not refine or g == 0 or g == len(b) - 1:
        return 0.0, None, None
    num, den = b[g - 1] - b[g + 1], b[g - 1] - 2.0 * b[g] + b[g + 1]
    return (sign * 0.5 * num / den if den < 0 else 0.0), den, num


def resolve(s, tab, k_max=2, relax_passes=2, min_rel=0.02, refine=True, picks=None, n_src=None):
    """The specification on one snapshot s [n_ch] (fp32 values) with Table tab.  picks[p][j]: the grid
    point of source j after the stages (p = 0) and after pass p, forced where given; n_src: the forced
    source count.  Returns a dict: flags, n_src, grid, pos, amp, total, residual, spectrum (B_0, or
    zeros), their bounds e_amp, e_pos (inf where ill-conditioned), e_total, e_residual, e_spectrum, and
    `why`: None, or why a forced pick or count cannot be what the specification gives."""
    s = np.asarray(s, np.complex64).astype(np.complex128)
    nch, ng = tab.n_ch, tab.n_grid
    out = dict(flags=FLAG_ONE_CH if nch == 1 else 0, n_src=0, grid=[], pos=[], amp=[], e_amp=[], e_pos=[],
               total=0.0, residual=0.0, e_total=0.0, e_residual=0.0, spectrum=np.zeros(ng), e_spectrum=np.zeros(ng),
               why=None, picked=[])
    if not np.all(np.isfinite(s)) or not np.any(s):
        out["flags"] |= FLAG_NO_SNAPSHOT
        out["picked"] = [[] for _ in range(relax_passes + 1)]
        return out
    defect = tab.defect
    r, e_rho, active = s.copy(), np.zeros(nch), {}
    out["total"] = float((np.abs(s) ** 2).sum())
    out["e_total"] = gamma(8) * out["total"]
    c_y = np.sqrt(2.0) * gamma(2 * nch)

    def err_r():
        return e_rho + sum((e_a * tab.abs[g] for e_a, g in active.values()), np.zeros(nch))

    def scan():
        e_r = err_r()
        y = (tab.a if defect == "unconjugated" else tab.a.conj()) @ r
        e_y = c_y * (tab.abs @ (np.abs(r) + e_r)) + tab.abs @ e_r
        ay = np.abs(y)
        b = ay ** 2 * tab.w
        e_b = tab.w * (2.0 * ay * e_y + e_y ** 2) + gamma(3) * tab.w * (ay + e_y) ** 2
        return y, e_y, b, e_b

    def best(b):
        return int(len(b) - 1 - np.argmax(b[::-1])) if defect == "highest_tie" else int(np.argmax(b))

    def fix(j, y, e_y, b, e_b, forced):
        """Source j from a scan: pick (forced or own), amplitude, position, cancellation."""
        nonlocal r, e_rho
        g_ref = best(b)
        g = g_ref if forced is None else int(forced)
        if b[g] < b[g_ref] - 2.0 * max(e_b[g], e_b[g_ref]) and out["why"] is None:
            out["why"] = f"source {j}: pick {g} has B {b[g]:.6g}, the maximum is {b[g_ref]:.6g} at {g_ref} (e_B {e_b[g]:.3g})"
        a = y[g] * tab.w[g]
        e_a = tab.w[g] * e_y[g] + U * abs(a)
        off, den, num = _parabola(b, g, refine, -1.0 if defect == "parabola_sign" else 1.0)
        e_pos = 2.0 * U * max(g, 1)
        if den is not None:
            e_num = e_b[g - 1] + e_b[g + 1] + U * abs(num)
            e_den = e_b[g - 1] + 2.0 * e_b[g] + e_b[g + 1] + 2.0 * U * (abs(b[g - 1]) + 2.0 * abs(b[g]) + abs(b[g + 1]))
            if e_den >= COND_MAX * abs(den):
                e_pos = np.inf
            else:
                e_pos += (0.5 * e_num + abs(off) * e_den) / (abs(den) - e_den)
        col, acol = tab.a[g], tab.abs[g]
        if defect != "no_subtraction":
            e_rho = e_rho + 2.0 * np.sqrt(2.0) * U * (np.abs(r) + err_r() + (abs(a) + e_a) * acol)
            active[j] = (e_a, g)
            r = r - a * col
        return g, off, a, e_a, e_pos

    def put_back(j):
        nonlocal r, e_rho
        a, e_a, g = out["amp"][j], out["e_amp"][j], out["grid"][j]
        acol = tab.abs[g]
        if defect != "no_subtraction":
            # each side adds back the very a_j A[g_j] it subtracted: that part of the distance goes as it came
            e_rho = e_rho + 2.0 * np.sqrt(2.0) * U * (np.abs(r) + err_r() + (abs(a) + e_a) * acol)
            del active[j]
            r = r + a * tab.a[g]

    b0 = e_b0 = 0.0
    for j in range(k_max):
        y, e_y, b, e_b = scan()
        g_ref = best(b)
        if j == 0:
            out["spectrum"], out["e_spectrum"] = b, e_b
            b0, e_b0 = b[g_ref], e_b[g_ref]
        top, e_top = b[g_ref], e_b.max()
        ends = top == 0.0 or (j > 0 and top < min_rel * b0)
        if n_src is not None:
            lim, e_lim = min_rel * b0, min_rel * e_b0 + U * min_rel * b0
            if j < n_src:      # the GPU went on
                if (top + e_top <= 0.0 or (j > 0 and top + e_top < lim - e_lim)) and out["why"] is None:
                    out["why"] = f"stage {j}: the search ends here (B {top:.6g}, limit {lim:.6g}), the GPU found {n_src}"
                ends = False
            else:              # the GPU ended here
                could = top - e_top <= 0.0 or (j > 0 and top - e_top < lim + e_lim)
                if not could and out["why"] is None:
                    out["why"] = f"stage {j}: the search goes on (B {top:.6g}, limit {lim:.6g}), the GPU found {n_src}"
                ends = True
        if ends:
            break
        forced = None if picks is None else picks[0][j]
        g, off, a, e_a, e_pos = fix(j, y, e_y, b, e_b, forced)
        for key, v in (("grid", g), ("pos", g + off), ("amp", a), ("e_amp", e_a), ("e_pos", e_pos)):
            out[key].append(v)
        out["n_src"] = j + 1
    out["picked"].append(list(out["grid"]))
    for p in range(relax_passes):
        for j in range(out["n_src"]):
            put_back(j)
            y, e_y, b, e_b = scan()
            forced = None if picks is None else picks[p + 1][j]
            g, off, a, e_a, e_pos = fix(j, y, e_y, b, e_b, forced)
            for key, v in (("grid", g), ("pos", g + off), ("amp", a), ("e_amp", e_a), ("e_pos", e_pos)):
                out[key][j] = v
        out["picked"].append(list(out["grid"]))
    ar, e_r = np.abs(r), err_r()
    out["residual"] = float((ar ** 2).sum())
    out["e_residual"] = float((2.0 * ar * e_r + e_r ** 2).sum() + gamma(8) * ((ar + e_r) ** 2).sum())
    return out


def resolve_list(snaps, steering, defect=None, **kw):
    """resolve() on every row of snaps [n][n_ch] without forced picks: a list of dicts."""
    tab = steering if isinstance(steering, Table) else Table(steering, defect)
    return [resolve(s, tab, **kw) for s in np.asarray(snaps)]


def assert_doa_match(runs, spectrum, snaps, steering, cells=None, label="", **cfg):
    """runs[p]: the GPU's DOA_DTYPE records with relax_passes = p, p = 0 .. cfg's relax_passes (the last is
    the run under test); spectrum: its float32 [n][n_grid] or None.  Every record against resolve() forced
    along the GPU's picks, within the module docstring's bounds.  Returns the worst fraction of each bound
    used: {"amp", "pos", "total", "residual", "spectrum", "cond" (worst compared E_den / |den| is below
    0.05 by construction; this is the share of sources skipped), "repicked" (records whose accepted picks
    differ from the unforced reference's)}."""
    tab = Table(steering)
    got = runs[-1]
    n = len(snaps)
    assert len(got) == n and len(runs) == cfg.get("relax_passes", 2) + 1, (len(got), n, len(runs))
    used = {"amp": 0.0, "pos": 0.0, "total": 0.0, "residual": 0.0, "spectrum": 0.0, "cond": 0.0, "repicked": 0}
    tiny = np.finfo(np.float64).tiny
    n_srcs = skipped = 0
    for i in range(n):
        g = got[i]
        if cells is None:
            assert g["frame"] == 0 and g["range"] == 0 and g["doppler"] == 0, f"{label} record {i}: cell fields without cells"
        else:
            assert (g["frame"], g["range"], g["doppler"]) == (cells[i]["frame"], cells[i]["range"], cells[i]["doppler"]), \
                f"{label} record {i}: cell fields"
        assert not np.any(g["reserved"]), f"{label} record {i}: reserved"
        k = int(g["n_src"])
        assert k <= cfg.get("k_max", 2), f"{label} record {i}: n_src {k}"
        assert all(int(run[i]["n_src"]) == k for run in runs), f"{label} record {i}: n_src differs between passes"
        assert g["src"][k:].tobytes() == bytes(16 * (4 - k)), f"{label} record {i}: sources beyond n_src are not zeros"
        picks = [[int(run[i]["src"]["grid"][j]) for j in range(k)] for run in runs]
        assert all(0 <= x < tab.n_grid for p in picks for x in p), f"{label} record {i}: grid out of range {picks}"
        ref = resolve(snaps[i], tab, picks=picks, n_src=k, **cfg)
        assert ref["why"] is None, f"{label} record {i}: {ref['why']}"
        assert int(g["flags"]) == ref["flags"] and k == ref["n_src"], f"{label} record {i}: flags {g['flags']}, n_src {k}"
        if picks != resolve(snaps[i], tab, **cfg)["picked"]:
            used["repicked"] += 1
        for key in ("total", "residual"):
            frac = abs(float(g[key]) - ref[key]) / max(ref["e_" + key], tiny)
            used[key] = max(used[key], frac)
            assert frac <= 1.0, f"{label} record {i}: {key} {g[key]} vs {ref[key]}: {frac:.3f} of its bound"
        if spectrum is not None:
            frac = float((np.abs(spectrum[i].astype(np.float64) - ref["spectrum"]) / np.maximum(ref["e_spectrum"], tiny)).max())
            used["spectrum"] = max(used["spectrum"], frac)
            assert frac <= 1.0, f"{label} record {i}: spectrum {frac:.3f} of its bound"
        for j in range(k):
            sj = g["src"][j]
            frac = abs(complex(sj["amp_re"], sj["amp_im"]) - ref["amp"][j]) / max(ref["e_amp"][j], tiny)
            used["amp"] = max(used["amp"], frac)
            assert frac <= 1.0, f"{label} record {i} source {j}: amplitude {frac:.3f} of its bound"
            n_srcs += 1
            if not np.isfinite(ref["e_pos"][j]):
                skipped += 1
                continue
            frac = abs(float(sj["pos"]) - ref["pos"][j]) / ref["e_pos"][j]
            used["pos"] = max(used["pos"], frac)
            assert frac <= 1.0, f"{label} record {i} source {j}: pos {sj['pos']} vs {ref['pos'][j]}: {frac:.3f} of its bound"
    used["cond"] = skipped / max(n_srcs, 1)
    assert skipped <= SKIP_SHARE * max(n_srcs, 1), f"{label} {skipped} of {n_srcs} sources ill-conditioned for pos"
    return used


def skipped_share(snaps, steering, **cfg):
    """The share of the reference's own sources whose parabola is ill-conditioned (e_pos infinite)."""
    e = [x for r in resolve_list(snaps, steering, **cfg) for x in r["e_pos"]]
    return float(np.mean(~np.isfinite(e))) if e else 0.0


# ---- scenes (tests/test_gpu_doa.py), checked on the CPU by tests/test_doa_host.py ----
def line_table(n_ch, n_grid, spacing=0.5):
    """fmcw.line_steering restated: (A complex64 [n_grid][n_ch], nu [n_grid] cycles per element)."""
    st = -1.0 + 2.0 * np.arange(n_grid) / n_grid
    return np.exp(2j * np.pi * spacing * st[:, None] * np.arange(n_ch)[None, :]).astype(np.complex64), spacing * st


def planted(n, n_ch, nus, amps, noise, seed, scale=1000.0):
    """n snapshots [n][n_ch] complex64 of a half-wavelength line array: sources at nus (cycles per
    element) with amplitudes amps times `scale` and a random phase each, Gaussian noise of `noise` times
    `scale` per component."""
    rng = np.random.default_rng(seed)
    k = np.arange(n_ch)
    s = noise * (rng.standard_normal((n, n_ch)) + 1j * rng.standard_normal((n, n_ch)))
    for nu, a in zip(nus, amps):
        s = s + a * np.exp(2j * np.pi * (nu * k[None, :] + rng.uniform(0, 1, (n, 1))))
    return (scale * s).astype(np.complex64)


def white(n, n_ch, seed, scale=1000.0):
    """White Gaussian snapshots: every record a hard case (no dominant source, near ties)."""
    rng = np.random.default_rng(seed)
    return (scale * (rng.standard_normal((n, n_ch)) + 1j * rng.standard_normal((n, n_ch)))).astype(np.complex64)


def phase_step_nu(s):
    """What fmcw_bearings reads from snapshots [n][n_ch]: arg(sum_k s_{k+1} conj(s_k)) / 2 pi."""
    s = np.asarray(s, np.complex128)
    return np.angle((s[:, 1:] * np.conj(s[:, :-1])).sum(axis=1)) / (2.0 * np.pi)


# The GPU matrix.  refine is on where the reference alone (test_doa_host.py) leaves at most 5 % of the
# sources to the parabola's skip: the small arrays and the 1024-point grid with one source, the others
# with a grid of at most 8 points per beamwidth.
GPU_CASES = [
    dict(n_ch=1, n_grid=64, k_max=1, relax_passes=0, refine=True, kind="white"),
    dict(n_ch=2, n_grid=64, k_max=1, relax_passes=0, refine=True, kind="white"),
    dict(n_ch=3, n_grid=128, k_max=4, relax_passes=2, refine=False, kind="white"),
    dict(n_ch=16, n_grid=64, k_max=2, relax_passes=2, refine=True, kind="white"),
    dict(n_ch=16, n_grid=128, k_max=2, relax_passes=2, refine=True, kind="planted", nus=(0.10, 0.22), amps=(1.0, 0.7)),
    dict(n_ch=16, n_grid=1024, k_max=4, relax_passes=2, refine=False, kind="white"),
    dict(n_ch=64, n_grid=1024, k_max=1, relax_passes=0, refine=True, kind="planted", nus=(-0.31,), amps=(1.0,)),
    dict(n_ch=64, n_grid=1024, k_max=4, relax_passes=2, refine=False, kind="planted", nus=(-0.2, 0.10, 0.13), amps=(1.0, 0.8, 0.6)),
    dict(n_ch=64, n_grid=128, k_max=2, relax_passes=2, refine=True, kind="white"),
]
GPU_RECORDS = 120


def case_id(c):
    return f"ch{c['n_ch']}-g{c['n_grid']}-k{c['k_max']}-p{c['relax_passes']}-{'refine' if c['refine'] else 'grid'}-{c['kind']}"


def gpu_case(c):
    """(snapshots, steering table, the resolver's keyword arguments) of one GPU case."""
    steering, _ = line_table(c["n_ch"], c["n_grid"])
    seed = 1000 + 7 * c["n_ch"] + c["n_grid"]
    if c["kind"] == "white":
        snaps = white(GPU_RECORDS, c["n_ch"], seed)
    else:
        snaps = planted(GPU_RECORDS, c["n_ch"], c["nus"], c["amps"], 0.01, seed)
    return snaps, steering, dict(k_max=c["k_max"], relax_passes=c["relax_passes"], refine=c["refine"], min_rel=0.02)


# The chain scene: two targets in one cell of a 16-element virtual array formed two ways.
CHAIN_ARRAYS = [(2, 8), (8, 2)]
CHAIN_NS, CHAIN_NC, CHAIN_CELL, CHAIN_NUS, CHAIN_GRID, CHAIN_SEED = 64, 256, (20, 5), (0.10, 0.22), 256, 4242
