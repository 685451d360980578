"""The TDM-MIMO virtual array's specification (include/fmcw.h, "TDM-MIMO virtual array") in fp64 NumPy,
and the tolerance the GPU tests hold fmcw_mimo_enqueue to.

    u_t[m]      = spec[f][k][r][m n_tx + t]                               t = 0 .. n_tx - 1, m = 0 .. n_d - 1
    none:         out[f][t n_rx + k][r][m] = u_t[m]                       (byte-exact)
    dft:          out[f][t n_rx + k][r][:] = ifft(fft(u_t) ramp_t),       ramp_t[q] = exp(-2 pi i s(q) t / (n_tx n_d)),
                  s = numpy.fft.fftfreq(n_d) n_d: the Nyquist bin takes the negative sign

Tolerance (assert_rows_match): per output row (f, v, r), |got - ref| <= MAP_TOL max |ref row|, the project's
map tolerance at the row's own scale: a delayed sequence has the scale of the sequence.
"""
import numpy as np

MAP_TOL = 1e-4


def split(spec, n_tx):
    """u [frame][t][rx][range][m] (a view where it can be): chirp c = m n_tx + t."""
    x = np.asarray(spec)
    nf, nrx, nr, nc = x.shape
    assert nc % n_tx == 0, (nc, n_tx)
    return x.reshape(nf, nrx, nr, nc // n_tx, n_tx).transpose(0, 4, 1, 2, 3)


def ramp(n_tx, n_d, nyquist_sign=-1, conj=False):
    """complex128 [t][q]: exp(-2 pi i s(q) t / (n_tx n_d)).  The two arguments open it to the modelled defects
    of tests/test_mimo_host.py (the Nyquist bin with the positive sign, the conjugated ramp)."""
    q = np.arange(n_d)
    s = np.where(q < n_d // 2, q, q - n_d)
    if nyquist_sign > 0:
        s[n_d // 2] = n_d // 2
    r = np.exp(-2j * np.pi * s[None, :] * np.arange(n_tx)[:, None] / (n_tx * n_d))
    return np.conj(r) if conj else r


def mimo_ref(spec, n_tx, align="dft", **ramp_kw):
    """out [frame][n_tx * n_rx][range][n_d] for spec [frame][rx][range][chirp]: complex128 for "dft"; for
    "none" the input's own values in its own dtype."""
    u = split(spec, n_tx)
    nf, _, nrx, nr, nd = u.shape
    if align == "dft":
        U = np.fft.fft(u.astype(np.complex128), axis=-1)
        u = np.fft.ifft(U * ramp(n_tx, nd, **ramp_kw)[None, :, None, None, :], axis=-1)
    else:
        assert align == "none", align
    return np.ascontiguousarray(u).reshape(nf, n_tx * nrx, nr, nd)


def mimo_f32(spec, n_tx):
    """The "dft" specification in complex64 (torch.fft on the CPU, the ramp rounded to complex64): what fp32
    rounding alone uses of the bound, to set a GPU figure against.  Not a second reference."""
    import torch
    u = np.ascontiguousarray(split(np.asarray(spec, np.complex64), n_tx))
    nf, _, nrx, nr, nd = u.shape
    r = torch.from_numpy(ramp(n_tx, nd).astype(np.complex64))[None, :, None, None, :]
    out = torch.fft.ifft(torch.fft.fft(torch.from_numpy(u), dim=-1) * r, dim=-1)
    return out.numpy().reshape(nf, n_tx * nrx, nr, nd)


def passes(ref, other):
    """The cells (a mask of ref's shape) in which `other` meets assert_rows_match's bound."""
    ref = np.asarray(ref, np.complex128)
    err = np.abs(np.broadcast_to(np.asarray(other, np.complex128), ref.shape) - ref)
    return err <= MAP_TOL * np.abs(ref).max(axis=-1, keepdims=True)


def unchecked_share(ref, other):
    """The share of the cells in which `other` (an array of ref's shape, or a scalar) passes the bound: the
    part of the output in which the tolerance cannot tell `other` from the reference."""
    return float(passes(ref, other).mean())


def bound_used(got, ref):
    """The worst fraction of assert_rows_match's bound that got uses."""
    got, ref = np.asarray(got), np.asarray(ref, np.complex128)
    assert got.shape == ref.shape, f"shape {got.shape}, expected {ref.shape}"
    assert np.all(np.isfinite(got.view(got.real.dtype))), "a value that is not finite"
    top = np.abs(ref).max(axis=-1)
    assert np.all(top > 0), "an all-zero reference row"
    return float((np.abs(got.astype(np.complex128) - ref).max(axis=-1) / (MAP_TOL * top)).max())


def assert_rows_match(got, ref, label=""):
    """got complex64 [frame][v][range][m] against mimo_ref's output.  Prints and returns the worst fraction
    of the bound used."""
    assert np.asarray(got).dtype == np.complex64, f"{label} dtype {np.asarray(got).dtype}"
    used = bound_used(got, ref)
    print(f"\n{label}: fraction of the bound used: {used:.3g}")
    assert used <= 1.0, f"{label} row error {used:.3f} of 1e-4 of the row's maximum"
    return used


# ---- the full-scale cases (tests/test_gpu_mimo.py), checked on the CPU by tests/test_mimo_host.py ----
FS_NR, FS_NF = 64, 3
FS_RXS = [1, 3]
FS_MATRIX = [(n_tx, n_d) for n_tx in (2, 4, 8) for n_d in (32, 64, 128, 256, 512) if n_tx * n_d <= 1024]
FS_LIMITS = [(32, 32, 2), (2, 32, 32), (1, 1024, 2)]       # (n_tx, n_d, n_rx) at the header's limits


def full_scale_case(n_tx, n_d, n_rx):
    """beams_ref.full_scale_spec for (FS_NF, n_rx, FS_NR, n_tx * n_d): white Gaussian, no quiet cell, so
    that the bound holds every output cell to 1e-4 of a scale that every cell has.  A raw sample of a later
    TX lies within the bound of its delayed value by chance in about one cell per million; with this seed
    base none of the 3-rx scenes has such a cell (tests/test_mimo_host.py asserts it on the reference)."""
    from beams_ref import full_scale_spec
    return full_scale_spec(FS_NF, n_rx, FS_NR, n_tx * n_d, seed=14000 + 100 * n_tx + 10 * n_rx + n_d)
