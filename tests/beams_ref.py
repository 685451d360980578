"""The beamformer's specification (include/fmcw.h, "Coherent beamforming") in fp64 NumPy, and the
tolerance the GPU tests hold fmcw_beams_enqueue to.

    y_b[c] = sum_k W[b][k] x_k[c]                     x_k[c] = spec[f][k][r][c]
    z_b    = the MTI canceller over y_b               (zero delay line before chirp 0)
    maps[f][b][r][d] = | fft_c(w[c] z_b[c])[d] |      w: bearings_ref.window

Tolerance (assert_maps_match): the project's map tolerance (tests/test_gpu_parity.py: 1e-4 of the
peak, and 1e-4 per bin above 1e-3 of the peak), taken at the scale BEFORE cancellation, because a
beam's null is a difference of channel terms and has no scale of its own:

    S[f, b, r, d] = sum_k |W[b][k]| |X_k[f, r, d]|,   X_k the per-channel Doppler spectrum (windowed,
                                                      cancelled) of this reference
    per (frame, beam):               max |gpu - ref| <= 1e-4 max S
    per bin with S > 1e-3 max S:     |gpu - ref|     <= 1e-4 S
"""
import numpy as np

from bearings_ref import MTI_COEF, _delayed, window

MAP_TOL = 1e-4
BIG = 1e-3


def channel_spectra(spec, win="hamming", mti=0):
    """X [frame][rx][range][doppler] complex128: the windowed, cancelled Doppler spectrum per channel."""
    x = np.asarray(spec).astype(np.complex128)
    m1, m2 = MTI_COEF[mti]
    y = x - m1 * _delayed(x, 1) + m2 * _delayed(x, 2)
    return np.fft.fft(y * window(x.shape[-1], win), axis=-1)


def beams_ref(spec, weights, win="hamming", mti=0):
    """(maps, S) as float64 [frame][beam][range][doppler] for spec [frame][rx][range][chirp] and
    weights [beam][rx]: the definition as the header writes it (the transform of the windowed,
    cancelled beam sum), and the scale from the channels' own spectra."""
    w = np.asarray(weights).astype(np.complex128)
    y = np.einsum("bk,fkrc->fbrc", w, np.asarray(spec).astype(np.complex128))
    maps = np.abs(channel_spectra(y, win, mti))
    S = np.einsum("bk,fkrd->fbrd", np.abs(w), np.abs(channel_spectra(spec, win, mti)))
    return maps, S


def bounds_used(got, ref, S):
    """The worst fraction of each bound of assert_maps_match that got uses: {"peak", "bin"}."""
    got = np.asarray(got)
    assert got.shape == ref.shape == S.shape, (got.shape, ref.shape, S.shape)
    assert got.dtype == np.float32 and np.all(np.isfinite(got))
    used = {"peak": 0.0, "bin": 0.0}
    err = np.abs(got.astype(np.float64) - ref)
    for f in range(ref.shape[0]):
        for b in range(ref.shape[1]):
            smax = S[f, b].max()
            assert smax > 0, f"{label} frame {f} beam {b}: an all-zero scale"
            used["peak"] = max(used["peak"], float(err[f, b].max() / (MAP_TOL * smax)))
            big = S[f, b] > BIG * smax
            used["bin"] = max(used["bin"], float((err[f, b][big] / (MAP_TOL * S[f, b][big])).max()))
    return used


def assert_maps_match(got, ref, S, label=""):
    """got float32 [frame][beam][range][doppler] against beams_ref's pair.  Prints and returns the
    worst fraction of each bound used: {"peak", "bin"}."""
    used = bounds_used(got, ref, S)
    print(f"\n{label}: fraction of each bound used: peak {used['peak']:.3g}, bin {used['bin']:.3g}")
    assert used["peak"] <= 1.0, f"{label} map error {used['peak']:.3f} of 1e-4 of the scale's peak"
    assert used["bin"] <= 1.0, f"{label} per-bin error {used['bin']:.3f} of 1e-4 of the bin's scale"
    return used


# ---- what the tolerance leaves unchecked, and a scene on which that is next to nothing -------------------
def passes(ref, S, other):
    """The cells (a mask of ref's shape) in which `other` meets both bounds of assert_maps_match."""
    err = np.abs(np.broadcast_to(np.asarray(other, np.float64), ref.shape) - ref)
    smax = S.max(axis=(2, 3), keepdims=True)
    return (err <= MAP_TOL * smax) & ((S <= BIG * smax) | (err <= MAP_TOL * S))


def unchecked_share(ref, S, other):
    """The share of the cells in which `other` (an array of ref's shape, or a scalar) passes both bounds
    of assert_maps_match against (ref, S): the part of the map in which the tolerance cannot tell `other`
    from the reference.  On a scene of a few tones over weak noise nearly every cell lies below
    1e-4 max S, and a zero, the neighbouring row or another frame's map passes there."""
    return float(passes(ref, S, other).mean())


def unchecked_shares(ref, S):
    """unchecked_share for the four maps a misplaced, stale or never-stored tile would leave behind:
    {"zero", "row" (the reference rolled by one range row), "frame", "beam" (the next frame's / beam's
    reference, cyclic; 1.0 where there is only one)}."""
    return {"zero": unchecked_share(ref, S, 0.0),
            "row": unchecked_share(ref, S, np.roll(ref, 1, axis=2)),
            "frame": unchecked_share(ref, S, np.roll(ref, -1, axis=0)),
            "beam": unchecked_share(ref, S, np.roll(ref, -1, axis=1))}


FULL_SCALE_RMS = 1000.0


def full_scale_spec(n_frames, n_rx, n_range, n_doppler, seed):
    """A spectrum [frame][rx][range][chirp] complex64 with no quiet cell: white Gaussian, rms
    FULL_SCALE_RMS per component, independent over frame, rx, row and chirp.  Its Doppler spectrum is
    white too, so under assert_maps_match every map cell is held to 1e-4 of its own scale (all but
    the canceller's null at Doppler 0: tests/test_beams_host.py measures the rest)."""
    rng = np.random.default_rng(seed)
    shape = (n_frames, n_rx, n_range, n_doppler)
    x = np.empty(shape, np.complex64)
    x.real = rng.standard_normal(shape, np.float32) * np.float32(FULL_SCALE_RMS)
    x.imag = rng.standard_normal(shape, np.float32) * np.float32(FULL_SCALE_RMS)
    x.setflags(write=False)
    return x


def beams_f32(spec, weights, win="hamming", mti=0):
    """The specification evaluated in float32 on the CPU (complex64 beam sum, canceller and window, a
    complex64 matrix DFT): what fp32 rounding alone uses of the bounds, to set a GPU figure against.
    Not a second reference: a matrix DFT adds n_doppler terms per bin where an FFT adds log2 of them."""
    x = np.asarray(spec, np.complex64)
    y = np.einsum("bk,fkrc->fbrc", np.asarray(weights, np.complex64), x).astype(np.complex64)
    m1, m2 = MTI_COEF[mti]
    z = (y - np.float32(m1) * _delayed(y, 1) + np.float32(m2) * _delayed(y, 2)).astype(np.complex64)
    nc = x.shape[-1]
    z *= window(nc, win).astype(np.float32)
    c = np.arange(nc)
    dft = np.exp(-2j * np.pi * ((c[:, None] * c[None, :]) % nc) / nc).astype(np.complex64)
    return np.abs((z.reshape(-1, nc) @ dft).reshape(z.shape)).astype(np.float32)


# ---- the full-scale GPU cases (tests/test_gpu_beams.py), checked on the CPU by tests/test_beams_host.py ----
FS_NR, FS_NF, FS_NB = 64, 2, 3
FS_DOPPLERS = [32, 64, 128, 256, 512, 1024]
FS_RXS = [1, 4]
FS_MTIS = [0, 2, 3]
FS_LIMITS = [(64, 3), (4, 64)]            # (n_rx, n_beams) at the header's limits, 64 x 32


def full_scale_case(nc, nrx, mti, nb=FS_NB):
    """(spec, weights, win) of a full-scale case: random complex weights, the window alternating over
    the matrix as test_gpu_beams.test_against_reference alternates it."""
    i, mi = FS_DOPPLERS.index(nc), FS_MTIS.index(mti)
    win = ("hamming", "none")[(i + mi + nrx // 2) % 2]
    spec = full_scale_spec(FS_NF, nrx, FS_NR, nc, seed=7000 + 10 * nc + nrx)
    rng = np.random.default_rng(100000 + 1000 * nc + 10 * nrx + mti + nb)
    w = (rng.standard_normal((nb, nrx)) + 1j * rng.standard_normal((nb, nrx))).astype(np.complex64)
    return spec, w, win
