"""The TDM-MIMO virtual array without a GPU: the C-ABI's layout, exports and argument checks (they come
before any device access), synth.tdm_frames, the float32 yardstick against the specification
(tests/mimo_ref.py), what the tolerance of the GPU tests can and cannot tell apart on their full-scale
scene, and the physics: the bearing of a moving target through the raw and the time-aligned array."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import fmcw_oracle as O
from fmcw import _lib as L
from fmcw import VirtualArray, synth
import bearings_ref as B
import mimo_ref as M

NEW_SYMBOLS = ("fmcw_mimo_config_default", "fmcw_mimo_create", "fmcw_mimo_destroy", "fmcw_mimo_enqueue",
               "fmcw_mimo_set_grid_for_test")
NAMES = ["n_range", "n_chirps", "n_rx", "n_tx", "align", "reserved", "device_id"]


def default_cfg(lib):
    cfg = L.FmcwMimoConfig()
    lib.fmcw_mimo_config_default(C.byref(cfg))
    return cfg


# ---- ABI -------------------------------------------------------------------------------------------
def test_layout_and_defaults(lib_built):
    assert C.sizeof(L.FmcwMimoConfig) == 32
    assert [f[0] for f in L.FmcwMimoConfig._fields_] == NAMES
    offsets = [0, 4, 8, 12, 16, 20, 28]
    assert [getattr(L.FmcwMimoConfig, n).offset for n in NAMES] == offsets
    src = L.HEADER_PATH.read_text()
    body = src[src.index("typedef struct fmcw_mimo_config {"):src.index("} fmcw_mimo_config;")]
    at = [body.index(n + ("[2];" if n == "reserved" else ";")) for n in NAMES]      # every field, in this order
    assert at == sorted(at)
    cfg = default_cfg(lib_built)
    assert (cfg.n_range, cfg.n_chirps, cfg.n_rx, cfg.n_tx) == (1024, 128, 4, 2)
    assert (cfg.align, list(cfg.reserved), cfg.device_id) == (L.MIMO_ALIGN_DFT, [0, 0], 0)
    assert (L.MIMO_ALIGN_NONE, L.MIMO_ALIGN_DFT) == (0, 1)
    assert "FMCW_MIMO_ALIGN_NONE = 0, FMCW_MIMO_ALIGN_DFT = 1" in src
    assert lib_built.fmcw_abi_version() == 8 and "Still 8 with the TDM-MIMO virtual array" in src


def test_new_symbols_exported(lib_built):
    out = subprocess.run(["nm", "-D", "--defined-only", str(L.LIB_PATH)], capture_output=True, text=True,
                         check=True).stdout
    src = L.HEADER_PATH.read_text()
    for name in NEW_SYMBOLS:
        assert f" T {name}\n" in out, name
        assert name in L.SIGNATURES and f"{name}(" in src


# (fields to set, the whole message), in the order fmcw_mimo_create checks them
BAD_FIELDS = [
    (dict(n_range=1000), b"n_range=1000: must be a power of two in [64, 8192]"),
    (dict(n_range=32), b"n_range=32: must be a power of two in [64, 8192]"),
    (dict(n_range=16384), b"n_range=16384: must be a power of two in [64, 8192]"),
    (dict(n_chirps=16), b"n_chirps=16: must be a power of two in [32, 1024]"),
    (dict(n_chirps=96), b"n_chirps=96: must be a power of two in [32, 1024]"),
    (dict(n_chirps=2048), b"n_chirps=2048: must be a power of two in [32, 1024]"),
    (dict(n_rx=0), b"n_rx=0: must be in [1, 64]"),
    (dict(n_rx=65, n_tx=1), b"n_rx=65: must be in [1, 64]"),
    (dict(n_tx=0), b"n_tx=0: must be a power of two in [1, 32]"),
    (dict(n_tx=3), b"n_tx=3: must be a power of two in [1, 32]"),
    (dict(n_tx=64, n_chirps=1024, n_rx=1), b"n_tx=64: must be a power of two in [1, 32]"),
    (dict(n_tx=8), b"n_tx=8: n_d = n_chirps / n_tx = 16, must be at least 32"),
    (dict(n_tx=32, n_chirps=512, n_rx=1), b"n_tx=32: n_d = n_chirps / n_tx = 16, must be at least 32"),
    (dict(n_tx=2, n_rx=33), b"n_tx=2 x n_rx=33: at most 64 virtual channels"),
    (dict(n_tx=32, n_chirps=1024, n_rx=3), b"n_tx=32 x n_rx=3: at most 64 virtual channels"),
    (dict(align=2), b"align 2 (0 NONE, 1 DFT)"),
    (dict(align=-1), b"align -1 (0 NONE, 1 DFT)"),
    (dict(reserved=(1, 0)), b"reserved {1, 0}: must be 0"),
    (dict(reserved=(0, 7)), b"reserved {0, 7}: must be 0"),
    (dict(device_id=-1), b"device_id -1 (0..63)"),
    (dict(device_id=64), b"device_id 64 (0..63)"),
]


@pytest.mark.parametrize("fields,msg", BAD_FIELDS, ids=[m.decode().split(":")[0].split(" (")[0] + f"#{i}"
                                                        for i, (_, m) in enumerate(BAD_FIELDS)])
def test_create_rejects_bad_fields(lib_built, fields, msg):
    """FMCW_EINVAL with the field's name, before any device access: the same answer on a machine without
    a GPU, and the handle stays null."""
    cfg = default_cfg(lib_built)
    for k, v in fields.items():
        if k == "reserved":
            cfg.reserved[0], cfg.reserved[1] = v
        else:
            setattr(cfg, k, v)
    h = C.c_void_p(1)
    assert lib_built.fmcw_mimo_create(C.byref(cfg), C.byref(h)) == L.FMCW_EINVAL
    assert lib_built.fmcw_last_error() == msg
    assert not h.value


def test_checks_come_in_the_header_order(lib_built):
    """With every field bad the first message; mending the fields one by one walks through the rest."""
    cfg = default_cfg(lib_built)
    cfg.n_range, cfg.n_chirps, cfg.n_rx, cfg.n_tx, cfg.align, cfg.device_id = 100, 100, 0, 3, 9, 99
    cfg.reserved[1] = 1
    steps = [(b"n_range", dict(n_range=64)), (b"n_chirps", dict(n_chirps=64)), (b"n_rx", dict(n_rx=33)),
             (b"n_tx=3", dict(n_tx=4)), (b"n_d", dict(n_tx=2)), (b"virtual channels", dict(n_rx=32)),
             (b"align", dict(align=0)), (b"reserved", dict()), (b"device_id", dict(device_id=0))]
    for want, mend in steps:
        h = C.c_void_p(1)
        assert lib_built.fmcw_mimo_create(C.byref(cfg), C.byref(h)) == L.FMCW_EINVAL and not h.value
        assert want in lib_built.fmcw_last_error(), (want, lib_built.fmcw_last_error())
        for k, v in mend.items():
            setattr(cfg, k, v)
        if want == b"reserved":
            cfg.reserved[1] = 0


def test_null_arguments(lib_built):
    assert lib_built.fmcw_mimo_create(None, None) == L.FMCW_EINVAL
    assert lib_built.fmcw_mimo_destroy(None) == L.FMCW_OK
    assert lib_built.fmcw_mimo_set_grid_for_test(None, 1) == L.FMCW_EINVAL
    assert lib_built.fmcw_last_error() == b"null virtual array"
    assert lib_built.fmcw_mimo_enqueue(None, None, 1, None, None) == L.FMCW_EINVAL
    lib_built.fmcw_mimo_config_default(None)


def test_create_without_device_fails_cleanly(lib_built):
    """The default configuration and the header's limits are valid: what is left is the device."""
    for fields in (dict(), dict(n_tx=32, n_chirps=1024, n_rx=2), dict(n_tx=2, n_rx=32, n_chirps=64),
                   dict(n_tx=1, n_chirps=1024, n_rx=64, align=0), dict(n_range=8192, n_chirps=1024, n_tx=4, n_rx=16)):
        cfg = default_cfg(lib_built)
        for k, v in fields.items():
            setattr(cfg, k, v)
        h = C.c_void_p(1)
        rc = lib_built.fmcw_mimo_create(C.byref(cfg), C.byref(h))
        if L.device_count() > 0:      # a valid configuration: the GPU tests take it from here
            assert rc == L.FMCW_OK and h.value, lib_built.fmcw_last_error()
            assert lib_built.fmcw_mimo_destroy(h) == L.FMCW_OK
        else:
            assert rc == L.FMCW_ENODEV and not h.value
            assert lib_built.fmcw_last_error() == b"no HIP device"


def test_python_class(lib_built):
    with pytest.raises(KeyError):
        VirtualArray(64, 64, 4, 2, align="fft")
    with pytest.raises(L.FmcwError, match="n_tx=3"):
        VirtualArray(64, 64, 4, 3)


# ---- synth.tdm_frames ------------------------------------------------------------------------------
def test_tdm_frames():
    """One transmitter is frames(); with more, chirp c carries the element phase of TX c mod n_tx, n_rx
    elements on: every (rx, chirp) line of a noiseless-enough scene is frames()'s line turned by it."""
    a = synth.tdm_frames(2, 64, 32, 3, 1, "two_targets", 77, [0.25, -0.125])
    assert a.dtype == np.complex64 and a.shape == (2, 3, 32, 64)
    assert np.array_equal(a, synth.frames(2, 64, 32, 3, "two_targets", 77, "f32", [0.25, -0.125]))
    ns, nc, nrx, ntx, p = 64, 64, 2, 4, 0.0625
    one = synth.tdm_frames(1, ns, nc, nrx, ntx, "random_target", 5, p).astype(np.complex128)
    flat = synth.frames(1, ns, nc, nrx, "random_target", 5, "f32", p).astype(np.complex128)
    turn = np.exp(2j * np.pi * p * nrx * (np.arange(nc) % ntx))[None, None, :, None]
    # noise +-100 and rounding against amplitude 20000: the lines agree to the noise, not exactly
    assert np.abs(one - flat * turn).max() <= 2 * np.sqrt(2) * 100 + 2
    assert np.abs(one).max() > 19000
    with pytest.raises(ValueError):
        synth.tdm_frames(1, 64, 32, 2, 3)
    with pytest.raises(ValueError):
        synth.tdm_frames(1, 64, 32, 2, 2, "two_targets", 1, [0.1])


# ---- the specification -----------------------------------------------------------------------------
def test_reference_closed_forms():
    """A tone at Doppler d (cycles per n_chirps chirps) below the per-TX Nyquist rate: the aligned output
    of TX t is TX 0's, the raw one is turned by 2 pi d t / n_chirps.  "none" returns the input's values;
    n_tx = 1 is the input."""
    ntx, nd, d = 4, 32, 5.3
    nc = ntx * nd
    c = np.arange(nc)
    spec = np.exp(2j * np.pi * d * c / nc)[None, None, None, :].astype(np.complex128)
    raw, out = M.mimo_ref(spec, ntx, "none"), M.mimo_ref(spec, ntx, "dft")
    assert raw.shape == out.shape == (1, ntx, 1, nd)
    for t in range(ntx):
        assert np.array_equal(raw[0, t, 0], spec[0, 0, 0, t::ntx])
        np.testing.assert_allclose(raw[0, t, 0], raw[0, 0, 0] * np.exp(2j * np.pi * d * t / nc), atol=1e-12)
    # a tone between bins leaks into every bin and the circular delay wraps at the ends: exact on a bin
    spec = np.exp(2j * np.pi * 8 * c / nc)[None, None, None, :]         # 8 cycles per 128: bin 2 of 32 per TX
    out = M.mimo_ref(spec, ntx, "dft")
    for t in range(ntx):
        np.testing.assert_allclose(out[0, t, 0], out[0, 0, 0], atol=1e-12)
    x = M.full_scale_case(2, 32, 3)
    assert M.mimo_ref(x, 2, "none").dtype == np.complex64
    assert np.array_equal(M.mimo_ref(x, 1, "none"), x)
    np.testing.assert_allclose(M.mimo_ref(x, 1, "dft"), x, atol=1e-9)
    v = M.mimo_ref(x, 2, "none")                                         # v = t n_rx + k
    assert np.array_equal(v[:, 1 * 3 + 2], x[:, 2, :, 1::2])
    np.testing.assert_allclose(M.mimo_ref(x, 2, "dft")[:, :3], v[:, :3], atol=1e-9)      # TX 0 is u_0


def test_assert_rows_match_counts_the_row_maximum():
    ref = np.zeros((1, 1, 2, 4), np.complex128)
    ref[0, 0, 0] = [1000, 10, 1, 0.01]
    ref[0, 0, 1] = [1, 1, 1, 1]
    got = ref.astype(np.complex64)
    assert M.assert_rows_match(got, ref) < 0.01
    assert M.unchecked_share(ref, 0.0) == 0.125                          # only 0.01 <= 1e-4 * 1000
    bad = got.copy()
    bad[0, 0, 1, 2] += 2e-4
    with pytest.raises(AssertionError):
        M.assert_rows_match(bad, ref)
    bad = got.copy()
    bad[0, 0, 0, 3] += 0.09                                              # 9e-5 of row 0's maximum
    assert 0.8 < M.assert_rows_match(bad, ref) <= 1.0
    with pytest.raises(AssertionError):
        M.assert_rows_match(got.astype(np.complex128), ref)


# ---- the yardstick ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n_tx,n_d", M.FS_MATRIX)
def test_float32_evaluation_of_the_full_scale_cases(n_tx, n_d):
    """mimo_ref.mimo_f32 (the specification in complex64 on the CPU) against the fp64 reference, on the
    scene of the GPU matrix: rounding alone stays below 1e-2 of the bound (measured: at most 3.0e-7 of
    the row maximum, 3.0e-3 of the bound)."""
    spec = M.full_scale_case(n_tx, n_d, 3)
    used = M.bound_used(M.mimo_f32(spec, n_tx), M.mimo_ref(spec, n_tx))
    print(f"\nfloat32 on the CPU, tx{n_tx} x {n_d}: {used:.3g} of the bound, {used * M.MAP_TOL:.3g} of the row maximum")
    assert used <= 1e-2


# ---- what the bound can tell apart -----------------------------------------------------------------
SHARE_CAP = 0.01
DEFECT_RX = 3


def v_swapped(ref, n_tx, n_rx):
    """The output with channel (t, k) stored at v = k n_tx + t."""
    out = np.empty_like(ref)
    for t in range(n_tx):
        for k in range(n_rx):
            out[:, k * n_tx + t] = ref[:, t * n_rx + k]
    return out


def defects(spec, n_tx, ref):
    """name -> the output a kernel with that defect would write."""
    return {
        "a zero": np.zeros_like(ref),
        "the neighbouring range row": np.roll(ref, 1, axis=2),
        "the neighbouring channel": np.roll(ref, 1, axis=1),
        "the raw de-interleave": M.mimo_ref(spec, n_tx, "none").astype(np.complex128),
        "the conjugated ramp": M.mimo_ref(spec, n_tx, conj=True),
        "the Nyquist bin with the positive sign": M.mimo_ref(spec, n_tx, nyquist_sign=+1),
        "v = k n_tx + t": v_swapped(ref, n_tx, spec.shape[1]),
        "slots shifted by one": M.mimo_ref(np.roll(spec, -1, axis=-1), n_tx),
    }


@pytest.mark.parametrize("n_tx,n_d", M.FS_MATRIX)
def test_full_scale_scene_is_checked_in_every_cell(n_tx, n_d):
    """On the full-scale scene of the GPU matrix (3 rx) each modelled defect passes assert_rows_match's
    bound in at most 1 % of the cells of the channels with t >= 1 (TX 0's rows are a copy either way).
    v = k n_tx + t leaves the channels with t (n_rx - 1) = k (n_tx - 1) where they are, the last one
    among them: it is measured on the channels it moves.  The raw copy and the conjugated ramp pass on
    TX 0's rows and nowhere else: 1 / n_tx of all cells, exactly.  On the reference alone."""
    nrx = DEFECT_RX
    spec = M.full_scale_case(n_tx, n_d, nrx)
    ref = M.mimo_ref(spec, n_tx)
    later = np.arange(n_tx * nrx) >= nrx                                 # t >= 1
    moved = np.array([(v % nrx) * n_tx + v // nrx != v for v in range(n_tx * nrx)])
    print()
    for name, other in defects(spec, n_tx, ref).items():
        ok = M.passes(ref, other)
        chans = later & moved if name.startswith("v =") else later
        share = float(ok[:, chans].mean())
        print(f"tx{n_tx} x {n_d} rx{nrx}: {name}: passes unnoticed in {100 * share:.4f} % of the cells")
        assert share <= SHARE_CAP, (name, share)
        if name in ("the raw de-interleave", "the conjugated ramp"):
            assert ok[:, ~later].all() and not ok[:, later].any(), name
            assert M.unchecked_share(ref, other) == 1.0 / n_tx


# ---- the physics -----------------------------------------------------------------------------------
# (n_tx, n_rx, n_chirps, synth seed of random_target, its Doppler in bins of one TX's n_d chirps, truth nu)
PHYSICS = [
    (2, 4, 128, 830, 9.29, 0.2),          # include/fmcw.h's example: 2 TX x 4 RX, n_d 64
    (8, 2, 512, 6055, 7.49, 0.03),        # 8 TX x 2 RX, n_d 64
    (2, 4, 128, 29422, 0.0, 0.2),         # (nearly) at rest: 0.0045 bins
]


@pytest.mark.parametrize("n_tx,n_rx,nc,seed,bins,truth", PHYSICS)
def test_bearing_through_the_virtual_array(n_tx, n_rx, nc, seed, bins, truth):
    """tdm_frames -> the oracle's range stage -> mimo_ref -> bearings_ref at the target's cell: the
    time-aligned array gives nu within 1e-3 of the truth at coherence >= 0.999; the raw de-interleave is
    off by at least 5e-3 wherever the target moves."""
    ns, nd = 64, nc // n_tx
    cube = synth.tdm_frames(1, ns, nc, n_rx, n_tx, "random_target", seed, truth)
    (r, d, _), = synth._targets("random_target", ns, nc, np.random.Generator(np.random.PCG64(seed)))[0]
    assert abs(d - bins) <= 0.01 and d < nd / 2                          # below half the per-TX PRF
    spec = O.range_ct(cube[0])[None]
    rec = np.zeros(1, np.dtype([("frame", "<u4"), ("range", "<u2"), ("doppler", "<u2")]))
    rec["range"], rec["doppler"] = int(round(r)), int(round(d)) % nd
    nu = {}
    for align in ("none", "dft"):
        got = B.bearings_ref(M.mimo_ref(spec, n_tx, align), rec)[0]
        nu[align], coh = float(got["nu"][0]), float(got["coherence"][0])
        print(f"\n{n_tx} TX x {n_rx} RX, {d:.2f} bins, {align}: nu {nu[align]:.4f} (truth {truth}), coherence {coh:.4f}")
    assert abs(nu["dft"] - truth) <= 1e-3 and coh >= 0.999
    if bins:
        assert abs(nu["none"] - truth) >= 5e-3
    else:
        assert abs(nu["none"] - truth) <= 1e-3
