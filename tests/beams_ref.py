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


def assert_maps_match(got, ref, S, label=""):
    """got float32 [frame][beam][range][doppler] against beams_ref's pair.  Prints and returns the
    worst fraction of each bound used: {"peak", "bin"}."""
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
    print(f"\n{label}: fraction of each bound used: peak {used['peak']:.3g}, bin {used['bin']:.3g}")
    assert used["peak"] <= 1.0, f"{label} map error {used['peak']:.3f} of 1e-4 of the scale's peak"
    assert used["bin"] <= 1.0, f"{label} per-bin error {used['bin']:.3f} of 1e-4 of the bin's scale"
    return used
