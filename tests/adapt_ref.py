"""The adaptive beam weights' specification (include/fmcw.h, "Adaptive beam weights") in fp64 NumPy, and
the bounds the GPU tests hold fmcw_adapt_enqueue to.

    z_k[c]  = the MTI canceller over spec[f][k][r][:]   (zero delay line before chirp 0)
    R[i][j] = (1/K) sum z_i conj(z_j)     over f, r in [train_r0, train_r0 + train_rows), every chirp
    delta   = loading * Re tr(R) / n_rx,  Rl = R + delta I
    W[b][k] = conj((Rl^-1 a_b)[k]) / (a_b^H Rl^-1 a_b)
    A[i][j] = (1/K) sum |z_i| |z_j|       the scale of the accumulation's error

Bounds.  The products are summed in fp32 in chains of at most L terms: a unit of the
accumulation holds ceil(T / n_units) steps of 64 snapshots, each added to the accumulator one
product at a time.  With the rounding of the canceller (2 operations per factor) and of the fp64
sum's conversion this is

    |R_gpu - R_ref|[i][j] <= gamma A[i][j],   gamma = C_SLACK (L + 4) 2^-24,
    L = 64 ceil(T / n_units),  T = n_frames ceil(train_rows n_doppler / 64),  n_units = min(T, 2048)

and, to first order in gamma, for every beam

    ||W_b - W_ref,b|| <= (4 ||Rl^-1||_2 gamma ||A||_F + 64 n_rx 2^-53 cond(Rl)) ||W_ref,b||

(the second term is the fp64 factorisation's; the rounding of W to fp32, 2^-24, is far inside the
first).  A case whose bound exceeds W_BOUND_MAX relative is a bad input and fails.
"""
import numpy as np

from bearings_ref import MTI_COEF, _delayed

FALLBACK = 1
PIVOT_MIN = 1e-8
MAX_UNITS = 2048
C_SLACK = 2.0
W_BOUND_MAX = 0.05


def chain_length(n_frames, train_rows, n_doppler):
    """(L, n_units): the longest fp32 add chain of the accumulation and the units of the call."""
    T = n_frames * -(-train_rows * n_doppler // 64)
    n_units = min(T, MAX_UNITS)
    return 64 * -(-T // n_units), n_units


def gamma(n_frames, train_rows, n_doppler):
    return C_SLACK * (chain_length(n_frames, train_rows, n_doppler)[0] + 4) * 2.0 ** -24


def snapshots(spec, mti=0, train_r0=0, train_rows=None):
    """z [rx][K] complex128 of spec [frame][rx][range][chirp]."""
    x = np.asarray(spec).astype(np.complex128)
    m1, m2 = MTI_COEF[mti]
    z = x - m1 * _delayed(x, 1) + m2 * _delayed(x, 2)
    r1 = x.shape[2] if train_rows is None else train_r0 + train_rows
    return z[:, :, train_r0:r1, :].transpose(1, 0, 2, 3).reshape(x.shape[1], -1)


def conventional(a):
    a = np.asarray(a).astype(np.complex128)
    return a.conj() / (np.abs(a) ** 2).sum(axis=1, keepdims=True)


def weights(R, a, loading):
    """(W, delta, flags, Rl) from a covariance: the loaded solve and the fallback of the header."""
    R = np.asarray(R, np.complex128)
    a = np.asarray(a).astype(np.complex128)
    n = R.shape[0]
    delta = float(loading) * float(np.trace(R).real) / n
    Rl = R + delta * np.eye(n)
    thr = PIVOT_MIN * float(np.trace(Rl).real) / n
    L = np.zeros((n, n), np.complex128)
    for j in range(n):                       # the Cholesky of the header, pivot by pivot
        s = Rl[j:, j] - L[j:, :j] @ L[j, :j].conj()
        if not s[0].real > thr:
            return conventional(a), delta, FALLBACK, Rl
        L[j, j] = np.sqrt(s[0].real)
        L[j + 1:, j] = s[1:] / L[j, j]
    x = np.linalg.solve(L.conj().T, np.linalg.solve(L, a.T))      # Rl^-1 a_b, one column per beam
    den = np.einsum("kb,kb->b", a.T.conj(), x).real
    W = (x / den).T.conj()
    flags = 0
    bad = ~np.isfinite(W.astype(np.complex64)).all(axis=1)
    if bad.any():
        W[bad] = conventional(a)[bad]
        flags = FALLBACK
    return W, delta, flags, Rl


def adapt_ref(spec, a, loading, mti=0, train_r0=0, train_rows=None):
    """dict(R, delta, W, flags, A, K, Rl) in fp64 for spec [frame][rx][range][chirp], a [beam][rx]."""
    z = snapshots(spec, mti, train_r0, train_rows)
    K = z.shape[1]
    R = z @ z.conj().T / K
    A = np.abs(z) @ np.abs(z).T / K
    W, delta, flags, Rl = weights(R, a, loading)
    return {"R": R, "delta": delta, "W": W, "flags": flags, "A": A, "K": K, "Rl": Rl}


def w_bound(ref, g):
    """The relative bound on ||W_b - W_ref,b|| for accumulation error g (above)."""
    n = ref["Rl"].shape[0]
    inv = np.linalg.norm(np.linalg.inv(ref["Rl"]), 2)
    return 4.0 * inv * g * np.linalg.norm(ref["A"]) + 64.0 * n * 2.0 ** -53 * np.linalg.cond(ref["Rl"])


def assert_matches(W, R, info, ref, g, loading, label=""):
    """The GPU's (W complex64, R complex128, parsed info) against adapt_ref's dict for a case without
    fallback; loading as the configuration holds it (fp32).  Prints and returns the worst fraction of
    each bound used: {"cov", "w"}."""
    assert W.dtype == np.complex64 and R.dtype == np.complex128
    assert np.all(np.isfinite(W)) and np.all(np.isfinite(R))
    assert info["K"] == ref["K"], (info["K"], ref["K"])
    assert info["flags"] == ref["flags"] == 0, (info["flags"], ref["flags"])
    assert np.array_equal(R, R.conj().T), "cov is not Hermitian bit for bit"
    used = {"cov": float((np.abs(R - ref["R"]) / (g * ref["A"])).max())}
    wb = w_bound(ref, g)
    rel = np.linalg.norm(W.astype(np.complex128) - ref["W"], axis=1) / np.linalg.norm(ref["W"], axis=1)
    used["w"] = float(rel.max() / wb)
    print(f"\n{label}: gamma {g:.3g}, W bound {wb:.3g} relative; fraction of each bound used: "
          f"cov {used['cov']:.3g}, w {used['w']:.3g}")
    assert wb <= W_BOUND_MAX, f"{label}: a bad input, the bound on W is {wb:.3g} relative"
    assert used["cov"] <= 1.0, f"{label}: cov error {used['cov']:.3f} of gamma A"
    assert used["w"] <= 1.0, f"{label}: W error {used['w']:.3f} of the perturbation bound"
    # delta: the fp64 formula on the GPU's own R, and within gamma of the reference's
    want = float(np.float32(loading)) * float(np.trace(R).real) / R.shape[0]
    assert abs(info["delta"] - want) <= 1e-12 * abs(want), (info["delta"], want)
    assert abs(info["delta"] - ref["delta"]) <= g * ref["delta"], (info["delta"], ref["delta"])
    return used


JAM_NR, JAM_NC, JAM_NRX = 64, 32, 8
JAM_CELL = (20, 5)            # the target's (range, doppler)
JAM_NU_T, JAM_NU_J = 0.1, -0.3


def jammer_scene(seed=7, nu_j=JAM_NU_J, nu_t=JAM_NU_T, jam_db=40.0, amp=1.0):
    """One frame [1][8][64][32] complex64 built directly as a spectrum: unit complex Gaussian noise per
    channel and cell; a jammer at nu_j cycles per element, white in range and chirp, jam_db above the
    noise; one target of amplitude amp per chirp at JAM_CELL and nu_t (amp 1: about 13.7 dB above the
    noise per channel after the Hamming-windowed Doppler sum: 20 log10(sum w / sqrt(sum w^2)))."""
    rng = np.random.default_rng(seed)
    def cn(*shape):
        return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) / np.sqrt(2.0)
    k = np.arange(JAM_NRX)[:, None, None]
    x = cn(JAM_NRX, JAM_NR, JAM_NC)
    x = x + 10.0 ** (jam_db / 20.0) * cn(JAM_NR, JAM_NC)[None] * np.exp(2j * np.pi * nu_j * k)
    r, d = JAM_CELL
    x[:, r, :] += amp * np.exp(2j * np.pi * (nu_t * k[:, :, 0] + d * np.arange(JAM_NC)[None, :] / JAM_NC))
    return np.ascontiguousarray(x[None].astype(np.complex64))


# ---- the GPU tests' shapes (tests/test_gpu_adapt.py), checked on the CPU by tests/test_adapt_host.py ----
NR = 64
DOPPLERS = [32, 1024]                     # the two ends of the chirp striding
RXS = [1, 2, 3, 4, 5, 8, 9, 15, 16]       # 8 | 9: the 16-row and the 32-row accumulator tile
MTIS = [0, 2, 3]
FRAMES = [1, 3]
# (train_r0, train_rows, loading): the whole map; one row; 3 rows (at n_doppler 32: 2 steps a frame,
# so 2 or 6 units, no multiple of a workgroup's 4 waves).  The short windows hold few snapshots per
# channel, so their loading is larger: the bound on W stays under W_BOUND_MAX.
WINDOWS = [(0, NR, 1e-3), (5, 1, 1e-1), (3, 3, 1e-1)]


def noise_scene(nd, nrx, seed=11):
    """3 frames [3][nrx][64][nd] complex64: unit complex Gaussian noise in every channel, an
    interferer at nu = 0.2 (10 dB, white in range and chirp) and static clutter (constant over the
    chirps, amplitude 3 in the rows 0 .. 7: the canceller removes it)."""
    rng = np.random.default_rng(seed + 1000 * nd + nrx)
    def cn(*shape):
        return ((rng.standard_normal(shape, np.float32) + 1j * rng.standard_normal(shape, np.float32))
                * np.float32(np.sqrt(0.5)))
    k = np.arange(nrx)[None, :, None, None]
    x = cn(3, nrx, NR, nd) + np.sqrt(10.0) * cn(3, 1, NR, nd) * np.exp(2j * np.pi * 0.2 * k)
    x[:, :, :8, :] += 3.0 * np.exp(2j * np.pi * 0.05 * k)
    x = np.ascontiguousarray(x.astype(np.complex64))
    x.setflags(write=False)
    return x


def case_constraints(nrx, nb, seed):
    """(steering vectors over (-0.5, 0.5), a random complex matrix: it catches a conjugated or
    transposed constraint)."""
    nus = (0.1 + np.arange(nb) / nb + 0.5) % 1.0 - 0.5
    k = np.arange(nrx)
    rng = np.random.default_rng(seed)
    rnd = (rng.standard_normal((nb, nrx)) + 1j * rng.standard_normal((nb, nrx))).astype(np.complex64)
    return np.exp(2j * np.pi * nus[:, None] * k[None, :]).astype(np.complex64), rnd


def matrix_case(nd, nrx, mti):
    """(n_frames, window) of a case of the main matrix: both alternate so that each meets every
    n_doppler, n_rx and MTI mode."""
    i = DOPPLERS.index(nd) + RXS.index(nrx) + MTIS.index(mti)
    return FRAMES[i % 2], WINDOWS[(i + RXS.index(nrx) // 3) % 3]


# ---- the full-scale cases: beams_ref.full_scale_spec, where the canceller's every output is at full scale ----
FS_NF = 2
FS_RXS = [4, 16]
FS_LOADING = 1e-3


def full_scale_case(nd, nrx, mti):
    """(spec, a): 2 frames of white Gaussian cells (the beamformer's full-scale scene: the whole map
    trains, so every row, frame and chirp of every channel counts in R with the same weight) and 3 random
    complex constraints."""
    from beams_ref import full_scale_spec
    return (full_scale_spec(FS_NF, nrx, NR, nd, seed=9000 + 10 * nd + nrx),
            case_constraints(nrx, 3, seed=500 + 1000 * nd + 10 * nrx + mti)[1])
