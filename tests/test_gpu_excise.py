"""The interference exciser on the GPU (fmcw_excise_* of libfmcw.so on gfx950 through the C-ABI).  The
repaired cube, the mask words, the counts and the status words are compared bit for bit with
tests/excise_ref.py (the header's specification in NumPy float32).  Every output buffer is filled with a
sentinel and carries canary space after it that must stay untouched.

Shapes are the smallest at which each mechanism can go wrong: Ns 64 (fewer samples than threads, one
pair of mask words) with the hand cases as lines; Ns 8192 (32 complex64 samples per thread, 256 mask
words) with bursts across word and wave boundaries; 30 lines of 1024 under 1 and 2 workgroups for the
persistent loop; Ns 256 of Rayleigh noise at alpha 1 for dense flags."""
import functools

import numpy as np
import pytest

import excise_ref as R
from fmcw import DeviceBuffer, InterferenceExciser, RadarCore, synth
from fmcw import _lib as L
from gpu_support import SENTINEL, Hip

pytestmark = pytest.mark.gpu

CANARY = 256         # sentinel bytes kept after every output
DTYPES = ("f32", "f16", "i16")


def as_dtype(z, dtype):
    """A complex cube in the conventions of `dtype`: complex64, float16 pairs (z / 4) or int16 pairs
    (z x 50, rounded)."""
    if dtype == "f32":
        return np.ascontiguousarray(z, np.complex64)
    iq = np.stack([z.real, z.imag], axis=-1)
    return np.rint(iq * 50).astype(np.int16) if dtype == "i16" else (iq / 4).astype(np.float16)


def filled(nbytes):
    buf = DeviceBuffer(nbytes + CANARY)
    buf.upload(np.full(nbytes + CANARY, SENTINEL, np.uint8))
    return buf


def tail_ok(buf, nbytes):
    return bool(np.all(buf.download(np.uint8, (CANARY,), offset=nbytes) == SENTINEL))


def run(ex, cube, in_place=False, want_mask=True, want_counts=True):
    """One fmcw_excise_enqueue on a host cube [frame][rx][chirp][sample]: (the repaired cube, the mask
    words or None, the counts or None, the status words), after checking the canaries."""
    cube = np.ascontiguousarray(cube)
    nf, lines, ns = cube.shape[0], int(np.prod(cube.shape[:3])), cube.shape[3]
    dc = filled(cube.nbytes)
    dc.upload(cube)
    do = dc if in_place else filled(cube.nbytes)
    dm = filled(lines * ns // 8) if want_mask else None
    dn = filled(lines * 4) if want_counts else None
    ds = filled(16)
    try:
        ex.enqueue(dc, nf, do, dm, dn, ds)
        st = ds.download(np.uint32, (4,))
        out = do.download(cube.dtype, cube.shape)
        mask = dm.download(np.uint32, cube.shape[:3] + (ns // 32,)) if want_mask else None
        counts = dn.download(np.uint32, cube.shape[:3]) if want_counts else None
        assert tail_ok(dc, cube.nbytes) and tail_ok(do, cube.nbytes) and tail_ok(ds, 16), "a canary was written"
        assert not want_mask or tail_ok(dm, lines * ns // 8), "the mask's canary was written"
        assert not want_counts or tail_ok(dn, lines * 4), "the counts' canary was written"
        if not in_place:
            assert dc.download(cube.dtype, cube.shape).tobytes() == cube.tobytes(), "the input cube was written"
    finally:
        for b in {id(b): b for b in (dc, do, dm, dn, ds) if b is not None}.values():
            b.free()
    return out, mask, counts, st


def check(cube, dtype, mode="zero", guard=4, rank_pct=50, alpha=16.0, label="", want=None, **kw):
    """The GPU against the reference on `cube`; returns the reference's outputs."""
    nf, nrx, nc, ns = cube.shape[:4]
    want = want or R.excise(cube, mode, guard, rank_pct, alpha)
    with InterferenceExciser(ns, nc, nrx, dtype, mode, guard, rank_pct, alpha, max_frames=nf) as ex:
        out, mask, counts, st = run(ex, cube, **kw)
    print(f"\n{label or mode} {dtype} {nf}x{nrx}x{nc}x{ns} guard {guard} rank {rank_pct} alpha {alpha}: status {want[3].tolist()}")
    assert st.tolist() == want[3].tolist()
    assert np.array_equal(counts, want[2])
    assert mask.tobytes() == R.mask_words(want[1]).tobytes()
    assert out.tobytes() == want[0].tobytes()
    return want


# ---- Ns 64: the hand cases as lines ---------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def hand_lines():
    """9 lines of 64 samples [3][1][3][64] complex128: a quiet line of power 2 with hot samples at both
    ends; two flags with 2 guard and with 2 guard + 1 clean samples between them (guard 4); isolated
    flags; flags at 16 and 48 (the whole line at guard 32); a line more than half zero (level 0); a line
    of tied powers 25 around the rank among powers 2; every inner sample hot (a run of Ns - 2 at guard
    0); a clean line."""
    ns = 64
    n = np.arange(ns)
    quiet = np.sqrt(2.0) * np.exp(2j * np.pi * n / 37.0) * 4
    lines = np.tile(quiet, (9, 1))
    for i, where in enumerate(([0, ns - 1], [20, 29], [20, 30], [7, 40], [16, 48])):
        lines[i, where] = 600.0
    lines[5] = 0
    lines[5, [3, 4, 30, 63]] = [1.0, 8 - 4j, 2j, 20.0]
    lines[6] = 1 - 1j
    tied = [3 + 4j, 5, -5j, -4 + 3j]
    for i, n0 in enumerate(range(0, 64, 8)):
        for j in range(5):
            lines[6, n0 + j] = tied[(i + j) % 4]
    lines[7, 1:-1] = 400 - 400j
    lines.setflags(write=False)
    return lines.reshape(3, 1, 3, ns)


@pytest.mark.parametrize("mode", [R.ZERO, R.INTERP])
@pytest.mark.parametrize("dtype", DTYPES)
def test_hand_cases_at_64_samples(gpu, dtype, mode):
    cube = as_dtype(hand_lines(), dtype)
    for guard, rank_pct, alpha in ((4, 50, 16.0), (0, 50, 16.0), (32, 50, 16.0), (0, 37, 2.0)):
        want = check(cube, dtype, mode, guard, rank_pct, alpha)
        g = want[1].reshape(9, 64)
        if (guard, rank_pct) == (4, 50):
            assert R.runs_of(g[0]) == [(0, 4), (59, 63)] and R.runs_of(g[1]) == [(16, 33)]
            assert R.runs_of(g[2]) == [(16, 24), (26, 34)] and not g[8].any()
            assert np.flatnonzero(g[5]).tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 8] + list(range(26, 35)) + [59, 60, 61, 62, 63]
        if (guard, rank_pct) == (0, 50):
            assert R.runs_of(g[3]) == [(7, 7), (40, 40)] and R.runs_of(g[7]) == [] and not g[6].any()
        if guard == 32:
            assert g[4].all() and not want[0].reshape(9, -1)[4].view(np.uint8).any() and want[3][3] >= 1
        if rank_pct == 37:
            assert g[6].sum() == 40                                  # the tied block, all of it
    want = check(cube, dtype, mode, 0, 1, 16.0, label=f"{mode} long run")   # the level is the smallest power
    assert R.runs_of(want[1].reshape(9, 64)[7]) == [(1, 62)]


# ---- Ns 8192: word and wave boundaries ------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def long_lines():
    """2 chirps of 8192 unit-noise samples; chirp 0 with bursts at samples 31..32, 63..64, 2047..2048, at
    0..2 and 8189..8191, and a run of 100 from 5000; chirp 1 with single hot samples 66 apart near 4096 (so
    that guard 32 leaves one clean sample between two runs) and a burst of 70 across 6143 / 6144."""
    rng = np.random.default_rng(8192)
    z = (rng.standard_normal((2, 8192)) + 1j * rng.standard_normal((2, 8192))) * np.sqrt(0.5) * 4
    for a, b in ((31, 32), (63, 64), (2047, 2048), (0, 2), (8189, 8191), (5000, 5099)):
        z[0, a:b + 1] += 300 * np.exp(2j * np.pi * 0.07 * np.arange(b + 1 - a))
    z[1, [4000, 4066, 4132]] += 300
    z[1, 6110:6180] += 300j
    z.setflags(write=False)
    return z.reshape(1, 1, 2, 8192)


@pytest.mark.parametrize("dtype,mode,guard", [("f32", R.INTERP, 32), ("f32", R.ZERO, 4), ("i16", R.INTERP, 4),
                                              ("f16", R.ZERO, 32), ("f16", R.INTERP, 0)])
def test_long_lines(gpu, dtype, mode, guard):
    want = check(as_dtype(long_lines(), dtype), dtype, mode, guard)
    g = want[1].reshape(2, 8192)
    runs = R.runs_of(g[0])
    assert runs[0][0] == 0 and runs[-1][1] == 8191 and max(b - a for a, b in runs) >= 99
    assert g[0, 31] and g[0, 32] and g[0, 63] and g[0, 64] and g[0, 2047] and g[0, 2048]
    if guard == 32:
        assert not g[1, 4033] and g[1, 4032] and g[1, 4034] and not g[1, 4099]


# ---- the persistent loop --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def burst_cube(dtype):
    """5 frames x 2 rx x 3 chirps of 1024 unit-noise samples, 12-sample bursts in every second chirp."""
    rng = np.random.default_rng(1024)
    z = (rng.standard_normal((5, 2, 3, 1024)) + 1j * rng.standard_normal((5, 2, 3, 1024))) * np.sqrt(0.5) * 4
    cube, truth = synth.interference_bursts(as_dtype(z, dtype), 2, 12, {"f32": 400.0, "f16": 100.0, "i16": 20000.0}[dtype], seed=7)
    cube.setflags(write=False)
    return cube, truth


@pytest.mark.parametrize("dtype", DTYPES)
def test_persistent_loop(gpu, dtype):
    """30 lines under 1 and 2 workgroups (30 and 15 lines each) and the built-in grid: identical bytes."""
    cube, truth = burst_cube(dtype)
    want = R.excise(cube, R.INTERP)
    assert want[3][1] >= 20 and not (truth & ~want[1]).any()          # chirps 0 and 2 of 10 (frame, rx), at least
    with InterferenceExciser(1024, 3, 2, dtype, R.INTERP, max_frames=5) as ex:
        for grid in (1, 2, 0):
            ex.set_grid_for_test(grid)
            out, mask, counts, st = run(ex, cube)
            assert st.tolist() == want[3].tolist() and np.array_equal(counts, want[2]), grid
            assert mask.tobytes() == R.mask_words(want[1]).tobytes() and out.tobytes() == want[0].tobytes(), grid
        out, mask, counts, st = run(ex, cube[:2])                     # fewer frames than max_frames
        assert out.tobytes() == want[0][:2].tobytes() and st[0] == want[2][:2].sum()


# ---- ranks and dense flags ------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def rayleigh_cube():
    rng = np.random.default_rng(256)
    z = (rng.standard_normal((2, 1, 4, 256)) + 1j * rng.standard_normal((2, 1, 4, 256))) * np.sqrt(0.5)
    z.setflags(write=False)
    return z


@pytest.mark.parametrize("rank_pct", [1, 50, 99])
def test_ranks_and_dense_flags(gpu, rank_pct):
    """alpha 1 on noise: the samples above the ranked one are flagged -- about 99 %, 50 % and 1 % of a
    line before the guard -- so most lines at ranks 1 and 50 count in status word 3."""
    for dtype, mode, guard in (("f32", R.INTERP, 1), ("i16", R.ZERO, 2), ("f16", R.INTERP, 4)):
        cube = as_dtype(rayleigh_cube() * 40, dtype)
        want = check(cube, dtype, mode, guard, rank_pct, 1.0)
        flagged = int(want[3][2])
        assert abs(flagged - 8 * (256 - 256 * rank_pct // 100 - 1)) <= (8 if dtype == "f32" else 64)   # ties in 16 bits
        assert want[3][3] == (8 if rank_pct < 99 else 0)


# ---- in place, NULL outputs -----------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_in_place_and_null_outputs(gpu, dtype):
    cube, _ = burst_cube(dtype)
    cube = cube[:2]
    want = R.excise(cube, R.INTERP)
    clean = as_dtype(rayleigh_cube(), dtype)
    assert R.excise(clean, R.INTERP)[3].tolist() == [0, 0, 0, 0]
    with InterferenceExciser(1024, 3, 2, dtype, R.INTERP, max_frames=2) as ex:
        for in_place in (False, True):
            for want_mask in (True, False):
                for want_counts in (True, False):
                    out, mask, counts, st = run(ex, cube, in_place, want_mask, want_counts)
                    assert out.tobytes() == want[0].tobytes() and st.tolist() == want[3].tolist()
                    assert mask is None or mask.tobytes() == R.mask_words(want[1]).tobytes()
                    assert counts is None or np.array_equal(counts, want[2])
    with InterferenceExciser(256, 4, 1, dtype, R.INTERP, max_frames=2) as ex:
        for in_place in (False, True):
            out, mask, counts, st = run(ex, clean, in_place)
            assert out.tobytes() == clean.tobytes() and st.tolist() == [0, 0, 0, 0]
            assert not mask.any() and not counts.any()


def test_argument_checks_with_a_device(gpu):
    lib = L.load()
    with InterferenceExciser(64, 2, max_frames=2) as ex:
        buf = filled(4096)
        p = buf.ptr
        for args, msg in (((None, 1, p, None, None, p + 2048), b"cube_dev"), ((p, 1, None, None, None, p + 2048), b"out_dev"),
                          ((p, 1, p, None, None, None), b"status_dev"), ((p, 0, p, None, None, p + 2048), b"n_frames"),
                          ((p, 3, p, None, None, p + 2048), b"n_frames"), ((p + 8, 1, p, None, None, p + 2048), b"cube_dev"),
                          ((p, 1, p + 16, None, None, p + 2048), b"overlaps")):
            assert lib.fmcw_excise_enqueue(ex._h, *args, None) == L.FMCW_EINVAL, args
            assert msg in lib.fmcw_last_error(), lib.fmcw_last_error()
        assert np.all(buf.download(np.uint8, (4096,)) == SENTINEL)
        buf.free()
        fixed, mask, counts, st = ex.repair(np.zeros((2, 1, 2, 64), np.complex64))
        assert fixed.shape == (2, 1, 2, 64) and mask.shape == (2, 1, 2, 64) and mask.dtype == bool
        assert counts.shape == (2, 1, 2) and st.tolist() == [0, 0, 0, 0]


# ---- the chain ------------------------------------------------------------------------------------
def e2e_cubes():
    """tests/test_excise_host.py's trial: 64 chirps x 256 samples of unit noise, a target of amplitude
    0.35 at (67, 5), 24-sample bursts of amplitude 100 in every second chirp."""
    nc, ns = 64, 256
    rng = np.random.default_rng(1)
    noise = (rng.standard_normal((nc, ns)) + 1j * rng.standard_normal((nc, ns))) * np.sqrt(0.5)
    n, c = np.arange(ns)[None, :], np.arange(nc)[:, None]
    clean = (noise + 0.35 * np.exp(2j * np.pi * (67 * n / ns + 5 * c / nc))).astype(np.complex64)[None, None]
    dirty, truth = synth.interference_bursts(clean, 2, 24, 100.0, seed=101)
    return clean, dirty, truth


@pytest.mark.parametrize("mode", [R.ZERO, R.INTERP])
def test_hand_off_to_the_chain(gpu, mode):
    """Exciser, then RadarCore with the 2-D OS-CFAR, both on the GPU: the repaired cube is the
    reference's, and the weak target is in the list only after the repair."""
    clean, dirty, truth = e2e_cubes()
    want = R.excise(dirty, mode)
    with InterferenceExciser(256, 64, mode=mode) as ex, RadarCore(N_RANGE=256, N_DOPPLER=64, cfar="os2d") as core:
        fixed, mask, counts, st = ex.repair(dirty)
        assert fixed.tobytes() == want[0].tobytes() and st.tolist() == want[3].tolist()
        assert np.array_equal(mask, want[1]) and np.array_equal(counts, want[2])

        def target(cube):
            d = core.process(cube).dets
            return (67, 5) in set(zip(d["range"].tolist(), d["doppler"].tolist()))
        assert not target(dirty) and target(fixed) and target(clean)


def test_graph_replay_in_front_of_the_chain(gpu):
    """fmcw_excise_enqueue (in place) and fmcw_enqueue captured once on one stream -- a linear chain --
    and replayed twice on fresh sentinel-filled outputs: both replays equal the direct call, status words
    included."""
    clean, dirty, truth = e2e_cubes()
    nr, nd, cap = 256, 64, 4096
    hip = Hip()
    with InterferenceExciser(nr, nd, mode=R.INTERP) as ex, RadarCore(N_RANGE=nr, N_DOPPLER=nd, cfar="os2d") as core:
        dc, dm, dk, dn = filled(dirty.nbytes), filled(nr * nd * 4), filled(nd * 4), filled(nr // 8 * nd)
        dd, ds, dst = filled(cap * 16), filled(16), filled(16)

        def calls(s):
            ex.enqueue(dc, 1, dc, dn, dk, dst, stream=s.value)
            core.enqueue(dc, 1, dm, dd, cap, ds, stream=s.value)

        def fresh():
            dc.upload(dirty)
            for b, n in ((dm, nr * nd * 4), (dk, nd * 4), (dn, nr // 8 * nd), (dd, cap * 16), (ds, 16), (dst, 16)):
                b.upload(np.full(n, SENTINEL, np.uint8))

        def result():
            for b, n in ((dc, dirty.nbytes), (dm, nr * nd * 4), (dk, nd * 4), (dn, nr // 8 * nd), (dd, cap * 16), (ds, 16),
                         (dst, 16)):
                assert tail_ok(b, n)
            n_dets = int(ds.download(np.uint32, (4,))[0])
            return (dc.download(np.uint8, (dirty.nbytes,)).tobytes(), dn.download(np.uint8, (nr // 8 * nd,)).tobytes(),
                    dk.download(np.uint32, (nd,)).tolist(), dst.download(np.uint32, (4,)).tolist(), n_dets,
                    dd.download(np.uint8, (n_dets * 16,)).tobytes(), dm.download(np.uint8, (nr * nd * 4,)).tobytes())
        try:
            with hip.graph(calls) as (exe, s):
                fresh()
                calls(s)
                hip.ok(hip.lib.hipStreamSynchronize(s))
                direct = result()
                want = R.excise(dirty, R.INTERP)
                assert direct[0] == want[0].tobytes() and direct[1] == R.mask_words(want[1]).tobytes()
                assert direct[2] == want[2].ravel().tolist() and direct[3] == want[3].tolist() and 0 < direct[4] <= cap
                for _ in range(2):
                    fresh()
                    hip.replay(exe, s)
                    assert result() == direct
        finally:
            for b in (dc, dm, dk, dn, dd, ds, dst):
                b.free()
