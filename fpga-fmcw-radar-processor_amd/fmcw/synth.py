"""Synthetic chirp cubes shaped like the reference's testbench stimuli.

x[c, n] = sum_k A_k exp(2 pi i (r_k n / Ns + d_k c / Nc)) + uniform noise, rounded and
saturated to the int16 ADC range, then stored as complex64 / f16 / int16 pairs.

  recipe "two_targets"  rtl/old/tb_radar_core.vhd:37-44, :106-129: targets (r = 100 Ns/1024,
                        d = +5, A = 8000) and (r = 500 Ns/1024, d = -10, A = 5000), noise +-20.
                        (Per-frame RNG: numpy PCG64, seed = seed + frame.)
  recipe "random_target" rtl/src/tb_radar_core.vhd:88-107: one target per frame at
                        r = U*0.88 Ns + 0.05 Ns, d = U*(100/128) Nc, A = 20000, noise +-100.
  phase offset per rx   2 pi rx rx_phase: a uniform line array sees a target at rx_phase cycles per
                        element (a scalar, or one value per target); default 0.25 (SURVEY.md 8d,
                        config 3), the bearing fmcw.bearings estimates back.

Used by bench.py and the tests; the product path never generates data itself.
"""
from __future__ import annotations

import numpy as np


def _targets(recipe: str, ns: int, nc: int, rng: np.random.Generator):
    if recipe == "two_targets":
        return [(100.0 * ns / 1024, 5.0, 8000.0), (500.0 * ns / 1024, -10.0, 5000.0)], 20.0
    if recipe == "random_target":
        r = rng.uniform() * 0.88 * ns + 0.05 * ns
        d = rng.uniform() * (100.0 / 128.0) * nc
        return [(r, d, 20000.0)], 100.0
    raise ValueError(recipe)


def frame(ns: int, nc: int, n_rx: int = 1, recipe: str = "two_targets", seed: int = 1234,
          dtype: str = "f32", rx_phase=0.25) -> np.ndarray:
    """One frame [rx][chirp][sample] as complex64 (f32), or [rx][chirp][sample][2] f16/int16.
    rx_phase: cycles per element, a scalar or one value per target of the recipe."""
    rng = np.random.Generator(np.random.PCG64(seed))
    tg, noise = _targets(recipe, ns, nc, rng)
    ph = [float(rx_phase)] * len(tg) if np.ndim(rx_phase) == 0 else [float(p) for p in rx_phase]
    if len(ph) != len(tg):
        raise ValueError(f"rx_phase has {len(ph)} values for the {len(tg)} targets of {recipe}")
    n = np.arange(ns)[None, :]
    c = np.arange(nc)[:, None]
    out = np.empty((n_rx, nc, ns), np.complex128)
    for rx in range(n_rx):
        x = np.zeros((nc, ns), np.complex128)
        for (r, d, a), p in zip(tg, ph):
            x += a * np.exp(2j * np.pi * (r * n / ns + d * c / nc + p * rx))
        x += noise * (rng.uniform(-1, 1, (nc, ns)) + 1j * rng.uniform(-1, 1, (nc, ns)))
        out[rx] = x
    i = np.clip(np.rint(out.real), -32768, 32767)
    q = np.clip(np.rint(out.imag), -32768, 32767)
    if dtype == "f32":
        return (i + 1j * q).astype(np.complex64)
    if dtype == "i16":
        return np.stack([i, q], axis=-1).astype(np.int16)
    if dtype == "f16":
        return (np.stack([i, q], axis=-1) / 32768.0).astype(np.float16)
    raise ValueError(dtype)


def frames(n_frames: int, ns: int, nc: int, n_rx: int = 1, recipe: str = "two_targets",
           seed: int = 1234, dtype: str = "f32", rx_phase=0.25) -> np.ndarray:
    return np.stack([frame(ns, nc, n_rx, recipe, seed + f, dtype, rx_phase) for f in range(n_frames)])


def tdm_frames(n_frames: int, ns: int, n_chirps: int, n_rx: int, n_tx: int, recipe: str = "two_targets",
               seed: int = 1234, rx_phase=0.25) -> np.ndarray:
    """frames() as a time-division MIMO front end records it: complex64 [frame][rx][chirp][sample], chirp
    c transmitted by TX c mod n_tx, the transmitters n_rx elements apart, so that receiver k sees the
    element phase 2 pi rx_phase (k + n_rx (c mod n_tx)) on chirp c: a uniform line array of n_tx * n_rx
    virtual elements.  The recipe's Doppler d stays in cycles per n_chirps chirps; one transmitter's n_d =
    n_chirps / n_tx chirps see d mod n_d.  The targets and the noise are frames()'s draws (per-frame seed
    = seed + frame): with n_tx = 1 the cube is frames()'s."""
    if n_tx < 1 or n_chirps % n_tx:
        raise ValueError(f"n_tx {n_tx}: n_chirps {n_chirps} must be a whole number of TX cycles")
    n = np.arange(ns)[None, :]
    c = np.arange(n_chirps)[:, None]
    out = np.empty((n_frames, n_rx, n_chirps, ns), np.complex128)
    for f in range(n_frames):
        rng = np.random.Generator(np.random.PCG64(seed + f))
        tg, noise = _targets(recipe, ns, n_chirps, rng)
        ph = [float(rx_phase)] * len(tg) if np.ndim(rx_phase) == 0 else [float(p) for p in rx_phase]
        if len(ph) != len(tg):
            raise ValueError(f"rx_phase has {len(ph)} values for the {len(tg)} targets of {recipe}")
        for rx in range(n_rx):
            x = np.zeros((n_chirps, ns), np.complex128)
            for (r, d, a), p in zip(tg, ph):
                x += a * np.exp(2j * np.pi * (r * n / ns + d * c / n_chirps + p * (rx + n_rx * (c % n_tx))))
            x += noise * (rng.uniform(-1, 1, (n_chirps, ns)) + 1j * rng.uniform(-1, 1, (n_chirps, ns)))
            out[f, rx] = x
    i = np.clip(np.rint(out.real), -32768, 32767)
    q = np.clip(np.rint(out.imag), -32768, 32767)
    return (i + 1j * q).astype(np.complex64)


def two_in_cell_frames(n_frames: int, ns: int, n_chirps: int, n_rx: int, n_tx: int, cell=(20, 5),
                       rx_phase=(0.10, 0.22), amps=(8000.0, 5600.0), noise: float = 20.0, seed: int = 1234) -> np.ndarray:
    """tdm_frames() with the targets given, all in one range-Doppler cell: complex64 [frame][rx][chirp]
    [sample], every target at range bin cell[0] and at Doppler cell[1] cycles per n_chirps chirps (an
    integer, so that one transmitter's n_chirps / n_tx chirps see bin cell[1] too), target q at rx_phase[q]
    cycles per element of the n_tx * n_rx virtual line array with amplitude amps[q] and a phase of its own
    (drawn per frame).  The bearing estimator reads one blended bearing there; the angle resolver reads
    them apart.  Uniform noise of +-noise per component, per-frame seed = seed + frame."""
    if n_tx < 1 or n_chirps % n_tx:
        raise ValueError(f"n_tx {n_tx}: n_chirps {n_chirps} must be a whole number of TX cycles")
    if len(rx_phase) != len(amps):
        raise ValueError(f"{len(rx_phase)} bearings for {len(amps)} amplitudes")
    n = np.arange(ns)[None, :]
    c = np.arange(n_chirps)[:, None]
    out = np.empty((n_frames, n_rx, n_chirps, ns), np.complex128)
    for f in range(n_frames):
        rng = np.random.Generator(np.random.PCG64(seed + f))
        phi = rng.uniform(0.0, 1.0, len(amps))
        for rx in range(n_rx):
            x = np.zeros((n_chirps, ns), np.complex128)
            for a, p, ph in zip(amps, rx_phase, phi):
                x += a * np.exp(2j * np.pi * (cell[0] * n / ns + cell[1] * c / n_chirps + p * (rx + n_rx * (c % n_tx)) + ph))
            x += noise * (rng.uniform(-1, 1, (n_chirps, ns)) + 1j * rng.uniform(-1, 1, (n_chirps, ns)))
            out[f, rx] = x
    i = np.clip(np.rint(out.real), -32768, 32767)
    q = np.clip(np.rint(out.imag), -32768, 32767)
    return (i + 1j * q).astype(np.complex64)


def interference_bursts(cube: np.ndarray, every: int, length: int, amplitude: float, seed: int, sweep: float = 0.002):
    """Mutual interference: another FMCW radar's chirp crossing ours.  In every `every`-th chirp (chirps
    0, every, 2 every, ...) of each frame and rx of `cube` -- complex [..., chirp, sample], or float16 /
    int16 [..., chirp, sample, 2] -- adds the burst amplitude exp(2 pi i (phi + f n + sweep n^2 / 2)),
    n = 0 .. length - 1, a linear FM crossing of `sweep` cycles per sample^2, at a random first sample in
    0 .. Ns - length, start frequency f in [-0.5, 0.5) cycles per sample and phase phi.  RNG: numpy
    PCG64 from `seed`; the first samples of all hit chirps, then their frequencies, then their phases,
    each in the cube's own order.  int16 cubes are rounded and saturated.

    Returns (a new cube of the same shape and dtype, true_mask bool [..., chirp, sample])."""
    cube = np.asarray(cube)
    pairs = not np.iscomplexobj(cube)
    z = (cube[..., 0] + 1j * cube[..., 1]) if pairs else cube.astype(np.complex128)
    z = np.array(z, np.complex128)
    nc, ns = z.shape[-2:]
    if not (1 <= length <= ns and every >= 1):
        raise ValueError(f"every {every}, length {length}: need every >= 1 and 1 <= length <= {ns}")
    rng = np.random.Generator(np.random.PCG64(seed))
    hit = np.arange(0, nc, every)
    shape = z.shape[:-2] + (len(hit),)
    first = rng.integers(0, ns - length + 1, shape)
    f0 = rng.uniform(-0.5, 0.5, shape)
    phi = rng.uniform(0.0, 1.0, shape)
    n = np.arange(length, dtype=np.float64)
    burst = amplitude * np.exp(2j * np.pi * (phi[..., None] + f0[..., None] * n + 0.5 * sweep * n * n))
    at = first[..., None] + np.arange(length)                     # [..., hit, length] sample indices
    true_mask = np.zeros(z.shape, bool)
    lead = np.indices(shape)
    idx = tuple(i[..., None] for i in lead[:-1]) + (hit[lead[-1]][..., None], at)
    z[idx] += burst
    true_mask[idx] = True
    if not pairs:
        return z.astype(cube.dtype), true_mask
    iq = np.stack([z.real, z.imag], axis=-1)
    if cube.dtype == np.int16:
        iq = np.clip(np.rint(iq), -32768, 32767)
    return iq.astype(cube.dtype), true_mask


def ieee_uniform(seed1: int, seed2: int, n: int):
    """IEEE 1076.2 MATH_REAL.UNIFORM (L'Ecuyer's combined multiplicative LCG, the RNG of every
    reference testbench): n draws from (seed1, seed2); returns (draws float64, seed1, seed2)."""
    out = np.empty(n, np.float64)
    s1, s2 = int(seed1), int(seed2)
    for k in range(n):
        s1 = (40014 * s1) % 2147483563     # = Schrage's form K := S/53668; 40014 (S - 53668 K) - 12211 K
        s2 = (40692 * s2) % 2147483399
        z = s1 - s2
        if z < 1:
            z += 2147483562
        out[k] = z * 4.656613e-10
    return out, s1, s2


def tb_radar_core_v3_cpis(n_cpi: int = 2, ns: int = 1024, nc: int = 128) -> np.ndarray:
    """The stimulus of rtl/old/tb_radar_core.vhd:86-141 (the testbench of radar_core_v3, the
    likely producer of data/radar_output.txt): targets (range 100, Doppler +5.0,
    amplitude 8000) and (500, -10.0, 5000) (:37-44), noise +-20 from UNIFORM with seeds (1, 1)
    drawn I then Q per sample (:121-124), VHDL integer() rounding (nearest, halves away from
    zero) and int16 saturation (:126-129), chirp-major, n_cpi CPIs.  Returns int16
    [cpi][chirp][sample][2] = (I, Q), the 32-bit AXI word {Q, I} (:131)."""
    n = np.arange(ns, dtype=np.float64)[None, :]
    c = np.arange(nc, dtype=np.float64)[:, None]
    ph1 = 2.0 * np.pi * (100.0 * n / ns + 5.0 * c / nc)
    ph2 = 2.0 * np.pi * (500.0 * n / ns + -10.0 * c / nc)
    i_t = 8000.0 * np.cos(ph1) + 5000.0 * np.cos(ph2)
    q_t = 8000.0 * np.sin(ph1) + 5000.0 * np.sin(ph2)
    draws, _, _ = ieee_uniform(1, 1, 2 * n_cpi * nc * ns)
    draws = draws.reshape(n_cpi, nc, ns, 2)
    i_acc = i_t[None] + 20.0 * (draws[..., 0] - 0.5) * 2.0
    q_acc = q_t[None] + 20.0 * (draws[..., 1] - 0.5) * 2.0

    def vhdl_int(x):
        return np.sign(x) * np.floor(np.abs(x) + 0.5)
    i = np.clip(vhdl_int(i_acc), -32768, 32767)
    q = np.clip(vhdl_int(q_acc), -32768, 32767)
    return np.stack([i, q], axis=-1).astype(np.int16)


def golden_chirp_frame(samples: np.ndarray, n_chirps: int = 128, n_samples: int = 256) -> np.ndarray:
    """BASELINE config 1 framing: data/golden_input_chirp.txt holds 2000 I/Q
    samples of one tone; a frame is n_chirps identical chirps = samples[0:n_samples]
    (a stationary target: all energy in Doppler bin 0)."""
    s = np.asarray(samples)
    z = (s[:n_samples, 0] + 1j * s[:n_samples, 1]).astype(np.complex64)
    return np.broadcast_to(z, (1, n_chirps, n_samples)).copy()


# ---- the tactical scenario (rtl/src/tb_tactical.vhd) ---------------------------------------------
# constants of tb_tactical.vhd:28-62 (QUICK_MODE column where the testbench has two)
TAC_WAVELENGTH = 0.1
TAC_MAX_RANGE_M = 120000.0
TAC_MACH_MPS = 340.29
TAC_NM_TO_M = 1852.0
TAC_SCAN_PERIOD = 1.0 / 2.0                  # SCAN_RATE 2 scans/s
TAC_PRF_HZ = (8000.0, 9000.0, 10000.0)
TAC_THERMAL_NOISE = 50.0
TAC_SEA_CLUTTER = 200.0
TAC_CLUTTER_RNG = 20000.0
TAC_RANGE_RES = 150.0
TAC_FTR_OFFSET = (0.0, -50.0, -50.0, -100.0, -100.0, -150.0)
TAC_CLAMP = 32000.0
# sea_scenario's own
SEA_CLUTTER_RHO = 0.9
SEA_LOW_FLYER_MPS = -60.0
# the low flyer's amplitude in ADC counts (the clutter of its range bin is about 190 counts rms):
# the fp64 oracle finds it in every scan behind the 2-pulse canceller and misses it in several
# scans with MTI off, at 128 x 32 and at 256 x 64 (tests/test_scenario_host.py holds both)
SEA_LOW_FLYER_AMP = 150.0


def _vhdl_int(x):
    """VHDL integer(real): nearest, halves away from zero."""
    return np.sign(x) * np.floor(np.abs(x) + 0.5)


def tac_rcs_to_amp(rcs: float, rng: float) -> float:
    """tb_tactical.vhd:158-162."""
    if rng < 1000.0:
        return 30000.0
    return float(np.sqrt(rcs) * 20000.0 / np.sqrt((rng / 10000.0) ** 4))


class _TacTargets:
    """The target states of tb_tactical.vhd:184-236: fighters at 45 NM in fingertip formation, Mach 1
    inbound, RCS 12; attackers at 39 NM, Mach 0.65, RCS 20.  step(scan) applies the notch (radial
    speed 0 from scan n_scans / 2 for three scans) and then the kinematics update of scan `scan`
    (1-based), as the testbench does before it generates that scan's returns."""

    def __init__(self, n_fighters: int, n_attackers: int, n_scans: int):
        self.ftr = [[45.0 * TAC_NM_TO_M + TAC_FTR_OFFSET[i % 6], -1.0 * TAC_MACH_MPS, 12.0, True]
                    for i in range(n_fighters)]
        self.att = [[39.0 * TAC_NM_TO_M, -0.65 * TAC_MACH_MPS, 20.0, True] for _ in range(n_attackers)]
        self.notch_scan = n_scans // 2

    def step(self, scan: int):
        if scan == self.notch_scan:
            for t in self.ftr:
                t[1] = 0.0
        elif scan == self.notch_scan + 3:
            for t in self.ftr:
                t[1] = -1.0 * TAC_MACH_MPS
        for t in self.ftr + self.att:
            t[0] = t[0] + t[1] * TAC_SCAN_PERIOD
            if t[0] < 5000.0:
                t[3] = False
        return [t for t in self.ftr + self.att if t[3]]     # (range_m, vel_radial, rcs, active)


def tb_tactical_scans(n_scans: int = 5, quick: bool = True):
    """The stimulus of rtl/src/tb_tactical.vhd:129-323, n_scans scans (NUM_SCANS; the notch is at
    n_scans / 2).  Per scan: PRF_HZ((scan - 1) mod 3), the notch and kinematics update (:213-236),
    then chirp outer / sample inner (:247-319): every active target whose range bin lies within 2
    samples of the fast-time index s adds amplitude (x 0.3 / |s - bin| off the bin) at phase
    2 pi (bin s / N_RANGE + doppler_bin c / N_DOPPLER) (:252-287; vel_to_doppler_bin adds
    N_DOPPLER / 2, :164-171); sea clutter while s x 150 < 20000 from two UNIFORM draws (:289-298);
    thermal noise from gauss (:149-156: two draws, u1 floored at 1e-10); clamp to +-32000
    (:306-309) and integer() rounding (:311-312).  All draws come from one ieee_uniform stream
    seeded (42, 42) that runs on from scan to scan.

    quick=True is the QUICK_MODE shape: 128 samples x 32 chirps, 2 fighters, 1 attacker.
    Returns (int16 [scan][1][chirp][sample][2] = (I, Q), truth): truth[scan] lists (range_bin,
    doppler_bin) per active target, fighters first."""
    ns, nc, n_ftr, n_att = (128, 32, 2, 1) if quick else (1024, 128, 6, 4)
    tg = _TacTargets(n_ftr, n_att, n_scans)
    s = np.arange(ns, dtype=np.float64)
    c = np.arange(nc, dtype=np.float64)[:, None]
    clut = s * TAC_RANGE_RES < TAC_CLUTTER_RNG                     # samples that take clutter draws
    # positions of a chirp's draws: clutter samples take 4 (amplitude, phase, u1, u2), the rest 2
    first = np.concatenate([[0], np.cumsum(np.where(clut, 4, 2))])
    per_chirp = int(first[-1])
    first = first[:-1]
    i_amp, i_ph = first[clut], first[clut] + 1
    i_u1 = first + np.where(clut, 2, 0)
    s1 = s2 = 42
    cubes = np.empty((n_scans, 1, nc, ns, 2), np.int16)
    truth = []
    for scan in range(1, n_scans + 1):
        prf = TAC_PRF_HZ[(scan - 1) % 3]
        acc = np.zeros((nc, ns), np.complex128)
        bins = []
        for rng_m, vel, rcs, _ in tg.step(scan):
            rb = int(_vhdl_int(rng_m / TAC_MAX_RANGE_M * ns))
            db = int(_vhdl_int(2.0 * vel / TAC_WAVELENGTH / prf * nc)) + nc // 2
            db += nc if db < 0 else -nc if db >= nc else 0
            bins.append((rb, db))
            off = np.abs(s - rb)
            amp = tac_rcs_to_amp(rcs, rng_m) * np.where(off == 0, 1.0, 0.3 / np.maximum(off, 1.0)) * (off < 3)
            acc += amp[None, :] * np.exp(2j * np.pi * (rb * s[None, :] / ns + db * c / nc))
        truth.append(bins)
        u, s1, s2 = ieee_uniform(s1, s2, nc * per_chirp)
        u = u.reshape(nc, per_chirp)
        sc = s[clut]
        amp = TAC_SEA_CLUTTER * (1.0 - sc / ns) * u[:, i_amp]
        ph = 2.0 * np.pi * (sc * sc / (ns * 10) + (u[:, i_ph] - 0.5) * 4.0 * c / nc)
        acc[:, clut] += amp * np.exp(1j * ph)
        u1 = np.maximum(u[:, i_u1], 1.0e-10)
        acc += TAC_THERMAL_NOISE * np.sqrt(-2.0 * np.log(u1)) * np.exp(2j * np.pi * u[:, i_u1 + 1])
        cubes[scan - 1, 0, ..., 0] = _vhdl_int(np.clip(acc.real, -TAC_CLAMP, TAC_CLAMP))
        cubes[scan - 1, 0, ..., 1] = _vhdl_int(np.clip(acc.imag, -TAC_CLAMP, TAC_CLAMP))
    return cubes, truth


def sea_clutter_edge(n_range: int) -> int:
    """First range bin without sea clutter: the testbench's 20 km of 120 km."""
    return int(round(n_range / 6))


def sea_clutter(rng: np.random.Generator, n_range: int, n_doppler: int) -> np.ndarray:
    """One scan's sea clutter [chirp][sample] complex128 (see sea_scenario): per range bin below the
    edge an AR(1) sequence over the chirps, drawn as standard_normal((edge, n_doppler, 2))."""
    edge = sea_clutter_edge(n_range)
    r = np.arange(edge, dtype=np.float64)
    w = rng.standard_normal((edge, n_doppler, 2))
    w = (w[..., 0] + 1j * w[..., 1]) * np.sqrt(0.5)                # unit variance
    g = np.empty((edge, n_doppler), np.complex128)
    g[:, 0] = w[:, 0]
    for k in range(1, n_doppler):
        g[:, k] = SEA_CLUTTER_RHO * g[:, k - 1] + np.sqrt(1.0 - SEA_CLUTTER_RHO ** 2) * w[:, k]
    to_fast = np.exp(2j * np.pi * r[:, None] * np.arange(n_range, dtype=np.float64)[None, :] / n_range)
    return (TAC_SEA_CLUTTER * (1.0 - r / n_range)[:, None] * g).T @ to_fast


def sea_scenario(n_range: int, n_doppler: int, n_scans: int, seed: int, low_flyer: bool = True):
    """tb_tactical's scenario (2 fighters, 1 attacker, the 3-PRF stagger, the notch at n_scans / 2
    for three scans) with its geometry meant in the range-bin domain:

      targets   tones over the whole chirp at the fractional range bin range_m / 120000 n_range
                and the fractional Doppler bin (2 v / 0.1 / prf n_doppler) mod n_doppler,
                amplitude tac_rcs_to_amp;
      clutter   for range bins r < edge = sea_clutter_edge(n_range): a complex Gaussian amplitude
                per chirp, AR(1) across chirps (rho 0.9, unit variance, stationary from chirp 0),
                times 200 (1 - r / n_range), brought to fast time by one matrix product with
                exp(2 pi i r n / n_range); nothing at or beyond edge;
      low flyer one more tone at range bin edge // 2 (it stays there), -60 m/s, SEA_LOW_FLYER_AMP;
      noise     Gaussian, sigma 50 per component; then clamp to +-32000 and integer() rounding.

    RNG: one numpy PCG64 generator from `seed` for the whole scene; per scan, in this order:
    standard_normal((edge, n_doppler, 2)) for the clutter's innovations (chirp 0 first), then
    standard_normal((n_doppler, n_range, 2)) for the noise.

    Returns (int16 [scan][1][chirp][sample][2], truth) as tb_tactical_scans does; truth holds the
    nearest bins (fighters, attacker, low flyer)."""
    ns, nc = n_range, n_doppler
    edge = sea_clutter_edge(ns)
    rng = np.random.Generator(np.random.PCG64(seed))
    tg = _TacTargets(2, 1, n_scans)
    n = np.arange(ns, dtype=np.float64)[None, :]
    c = np.arange(nc, dtype=np.float64)[:, None]
    cubes = np.empty((n_scans, 1, nc, ns, 2), np.int16)
    truth = []
    for scan in range(1, n_scans + 1):
        prf = TAC_PRF_HZ[(scan - 1) % 3]
        tones = [(rng_m / TAC_MAX_RANGE_M * ns, vel, tac_rcs_to_amp(rcs, rng_m)) for rng_m, vel, rcs, _ in tg.step(scan)]
        if low_flyer:
            tones.append((float(edge // 2), SEA_LOW_FLYER_MPS, SEA_LOW_FLYER_AMP))
        acc = np.zeros((nc, ns), np.complex128)
        bins = []
        for rb, vel, amp in tones:
            db = (2.0 * vel / TAC_WAVELENGTH / prf * nc) % nc
            bins.append((int(round(rb)), int(round(db)) % nc))
            acc += amp * np.exp(2j * np.pi * (rb * n / ns + db * c / nc))
        truth.append(bins)
        acc += sea_clutter(rng, ns, nc)
        w = rng.standard_normal((nc, ns, 2))
        acc += TAC_THERMAL_NOISE * (w[..., 0] + 1j * w[..., 1])
        cubes[scan - 1, 0, ..., 0] = _vhdl_int(np.clip(acc.real, -TAC_CLAMP, TAC_CLAMP))
        cubes[scan - 1, 0, ..., 1] = _vhdl_int(np.clip(acc.imag, -TAC_CLAMP, TAC_CLAMP))
    return cubes, truth
