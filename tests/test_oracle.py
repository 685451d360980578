"""Pin the CPU oracle against the reference's own known-answer tests and data files.

Every check here restates a reference testbench assertion or a property of a reference data
file (citations inline).  No GPU needed.
"""
import json

import numpy as np
import pytest

import fmcw_oracle as O
from conftest import GOLDEN


def test_magnitude_kat_exact():
    """rtl/src/tb_magnitude_calc.vhd:49-73 vectors vs its model :32-40 (checked within 1 LSB
    at :156-166; the integer model is exact)."""
    kat = json.loads((GOLDEN / "mag_kat.json").read_text())
    i = np.array([k["i"] for k in kat])
    q = np.array([k["q"] for k in kat])
    exp = np.array([k["expect"] for k in kat])
    np.testing.assert_array_equal(O.ambm(i, q), exp)
    spot = {(1000, 1000): 1375, (5000, 3000): 6125, (-8000, 6000): 10250, (32000, 32000): 44000,
            (1, 1): 1, (30000, 100): 30037}
    for (a, b), v in spot.items():
        assert int(O.ambm(a, b)) == v


def test_corner_turn_kat():
    """rtl/src/tb_corner_turner.vhd:36-49,146-186: output (range r, Doppler d) decodes to
    chirp = d, sample = r; emitted range-major (corner_turner.vhd:80)."""
    z = np.load(GOLDEN / "ct_kat.npz")
    cm = z["chirp_major"]
    out = np.swapaxes(cm[None].astype(np.complex128), -1, -2)[0].real.astype(np.int64)  # the CT
    np.testing.assert_array_equal(out, z["range_major"])
    for r in range(out.shape[0]):
        for d in range(out.shape[1]):
            assert out[r, d] // 256 == d and out[r, d] % 256 == r
    # emission order: linear read index = range * N_DOPPLER + doppler walks range-major
    flat = out.ravel()
    assert list(flat[:3]) == [0 * 256 + 0, 1 * 256 + 0, 2 * 256 + 0]


def test_window_tables_and_tb_checks():
    """Hamming ROM (window_multiplier.vhd:34-49) + tb_window_multiplier.vhd:182-240 checks."""
    w = json.loads((GOLDEN / "window.json").read_text())
    for n in (64, 128, 256, 1024):
        np.testing.assert_array_equal(O.hamming_q15(n), np.array(w[str(n)]["q15_rom"]))
        f = O.window_f32(n)
        np.testing.assert_array_equal(f, np.array(w[str(n)]["f32"], np.float32))
        assert np.array_equal(f, f[::-1])                     # symmetric (mirrored ROM)
    n = 64
    dc = 16000.0 * O.window_f32(n)                             # Test 1: DC 16000
    assert abs(dc[0]) <= 3000 and abs(dc[-1]) <= 3000 and abs(dc[n // 2]) >= 10000
    assert np.all(0.0 * O.window_f32(n) == 0)                  # Test 2: zero in -> zero out
    # the RTL arithmetic (>>14, +2^14) is a 2x gain with +1 LSB: zero in gives 1
    assert np.all(O.window_q15_rtl(np.zeros(n, np.int64), n) == 1)
    y = O.window_q15_rtl(np.full(n, 8000), n)                  # Test 5: symmetry within +-1
    assert np.all(np.abs(y - y[::-1]) <= 1)


def test_golden_chirp_peaks():
    """data/golden_input_chirp.txt: one tone at 17/60 cycles/sample; FFT peaks pin direction
    and ordering (forward, natural): 128-pt bin 36, 256-pt bin 73, 1024-pt bin 290."""
    iq = np.loadtxt(GOLDEN / "golden_input_chirp.txt", dtype=np.int64)
    assert iq.shape == (2000, 2)
    z = iq[:, 0] + 1j * iq[:, 1]
    mag = np.abs(z)
    assert 16300 < mag.min() and mag.max() < 16500
    for n, b in ((128, 36), (256, 73), (1024, 290)):
        spec = np.fft.fft(z[:n])
        assert int(np.argmax(np.abs(spec))) == b
        # the oracle's range FFT (window off) is the same transform
        rc = O.range_ct(z[None, :n], window=False)[:, 0]
        np.testing.assert_allclose(rc, spec, rtol=0, atol=1e-6 * np.abs(spec).max())


def test_golden_chirp_c1_fixture():
    """BASELINE config 1 (128 chirps x 256 samples): stored oracle outputs reproduce."""
    z = np.load(GOLDEN / "golden_chirp_c1.npz")
    res = O.process(z["cube"], O.Cfar1D())
    np.testing.assert_allclose(res["mag"], z["mag"], rtol=1e-12, atol=1e-9)
    np.testing.assert_array_equal(res["dets"], z["dets_os1d"])
    r, d = np.unravel_index(np.argmax(res["mag"]), res["mag"].shape)
    assert (r, d) == (73, 0)           # stationary tone: range bin 73, zero Doppler


@pytest.mark.slow
def test_radar_output_coarse_invariants():
    """data/radar_output.txt pins only coarse invariants: its target energy
    sits in range rows 99-101 and 499-501 for the rtl/old/tb_radar_core.vhd:37-44 stimulus.
    The oracle on that stimulus must put its energy in the same rows."""
    prof = np.load(GOLDEN / "radar_output_profile.npz")
    top = set(prof["top_rows"].tolist())
    assert top == {99, 100, 101, 499, 500, 501}
    # stimulus: 1024 x 128, targets (100, +5, 8000) and (500, -10, 5000), noise +-20
    ns, nc = 1024, 128
    n = np.arange(ns)[None, :]
    c = np.arange(nc)[:, None]
    x = 8000 * np.exp(2j * np.pi * (100 * n / ns + 5.0 * c / nc)) + \
        5000 * np.exp(2j * np.pi * (500 * n / ns - 10.0 * c / nc))
    rng = np.random.default_rng(1)
    x = x + 20 * (rng.uniform(-1, 1, x.shape) + 1j * rng.uniform(-1, 1, x.shape))
    x = np.clip(np.rint(x.real), -32768, 32767) + 1j * np.clip(np.rint(x.imag), -32768, 32767)
    mag = O.process(x.astype(np.complex64), None)["mag"]
    ours = np.argsort(-mag.sum(axis=1))[:6]
    assert set(ours.tolist()) == top
    # natural Doppler order: +5 -> bin 5, -10 -> bin 118
    assert int(np.argmax(mag[100])) == 5 and int(np.argmax(mag[500])) == 118


def test_tb_cfar2d_map():
    """rtl/src/tb_os_cfar_2d.vhd:52-75 map; the testbench asserts >= 2 detections
    (:132-134, :207-209).  The oracle finds both targets and reproduces the fixture."""
    z = np.load(GOLDEN / "tb_cfar2d.npz")
    rr, gr, rd, gd = z["params"].tolist()
    p = O.Cfar2D(ref_range=rr, guard_range=gr, ref_doppler=rd, guard_doppler=gd)
    assert p.n_ref == (2 * 3 + 1) * (2 * 4 + 1) - 3 * 3
    det, thr = O.cfar_os2d(z["map"].astype(np.float32), p)
    dets = O.detections(det, z["map"].astype(np.float32), thr)
    np.testing.assert_array_equal(dets, z["dets"])
    assert len(dets) >= 2
    pos = set(zip(dets["range"].tolist(), dets["doppler"].tolist()))
    assert (30, 16) in pos and (50, 8) in pos


def test_mti_tb_doppler_notch_checks():
    """rtl/src/tb_doppler_notch.vhd:95-180 (N_DOPPLER 32, amplitude 10000): 2-pulse nulls DC
    (only the first sample after the reset survives), passes an f=8 tone (avg |y| >= 1000,
    :139), bypass passes DC (>= 5000, :156), 3-pulse nulls DC, the delay line resets at each
    sequence (:99-102).  Checked on the fp restatement and on the int16 RTL-compat form."""
    n = 32
    s = np.arange(n)

    def chirp(f):
        ph = 2 * np.pi * f * s / n
        return np.rint(10000 * np.cos(ph)), np.rint(10000 * np.sin(ph))

    for mode in (2, 3):
        i, q = chirp(0.0)
        y = O.mti((i + 1j * q)[None], mode)[0]
        assert np.all(np.abs(y[mode - 1 + (mode == 3):]) == 0) and abs(y[0]) == 10000
        yi, yq = O.mti_rtl_int16(i, q, mode)
        np.testing.assert_array_equal(yi + 1j * yq, y)
    i, q = chirp(8.0)
    y2 = O.mti((i + 1j * q)[None], 2)[0]
    assert np.mean(np.abs(y2)) >= 1000
    i, q = chirp(0.0)
    assert np.mean(np.abs(O.mti((i + 1j * q)[None], 0)[0])) >= 5000
    # reset: two bursts processed as two range bins give identical outputs
    two = np.stack([i + 1j * q, i + 1j * q])
    out = O.mti(two, 2)
    np.testing.assert_array_equal(out[0], out[1])
    # saturation exists only in the int16 compat form
    yi, _ = O.mti_rtl_int16(np.array([32767, -32768]), np.array([0, 0]), 2)
    assert list(yi) == [32767, -32768]


def test_cfar_defaults_match_reference_generics():
    """os_cfar_2d as instantiated (radar_core.vhd:376-382): 11 x 13 window, 128 refs, k=96;
    os_cfar 1-D (radar_core_v3.vhd:373-381): 16 refs, k=12, alpha 4."""
    p = O.Cfar2D()
    assert p.n_ref == 128 and p.rank == 96
    assert len(O.cfar2d_offsets(p)) == 128
    q = O.Cfar1D()
    assert 2 * q.ref == 16 and q.rank == 12 and q.alpha == 4.0


def test_tb_radar_core_v3_stimulus_invariants():
    """The exact rtl/old/tb_radar_core.vhd:86-141 stimulus (IEEE UNIFORM noise, seeds 1/1, two
    CPIs) through the oracle: both CPIs put their energy in the rows data/radar_output.txt
    carries (99-101, 499-501), with Doppler peaks at natural bins 5 and 118."""
    from fmcw import synth
    cpis = synth.tb_radar_core_v3_cpis()
    assert cpis.shape == (2, 128, 1024, 2) and cpis.dtype == np.int16
    top = set(np.load(GOLDEN / "radar_output_profile.npz")["top_rows"].tolist())
    for k in range(2):
        x = cpis[k].astype(np.float64)
        mag = O.process(x[..., 0] + 1j * x[..., 1], None)["mag"]
        assert set(np.argsort(-mag.sum(axis=1))[:6].tolist()) == top
        assert int(np.argmax(mag[100])) == 5 and int(np.argmax(mag[500])) == 118
    # noise stays inside +-20 of the two tones (VHDL integer() rounding, no saturation)
    n = np.arange(1024)[None, :]
    c = np.arange(128)[:, None]
    tone = 8000 * np.exp(2j * np.pi * (100 * n / 1024 + 5 * c / 128)) + \
        5000 * np.exp(2j * np.pi * (500 * n / 1024 - 10 * c / 128))
    x = cpis[0].astype(np.float64)
    assert np.abs(x[..., 0] - tone.real).max() <= 20.5 and np.abs(x[..., 1] - tone.imag).max() <= 20.5


def test_ieee_uniform_recurrence():
    """MATH_REAL.UNIFORM: L'Ecuyer's two MLCGs (40014 mod 2147483563, 40692 mod 2147483399) in
    (0, 1); Schrage's decomposition used by the VHDL body equals the direct product."""
    from fmcw import synth
    u, s1, s2 = synth.ieee_uniform(1, 1, 1000)
    assert np.all((u > 0) & (u < 1)) and abs(u.mean() - 0.5) < 0.05
    assert (s1, s2) == (pow(40014, 1000, 2147483563), pow(40692, 1000, 2147483399))
    t1 = 123456789
    k = t1 // 53668
    schrage = 40014 * (t1 - k * 53668) - k * 12211
    assert (schrage + 2147483563 if schrage < 0 else schrage) == (40014 * t1) % 2147483563


def test_rtl_compat_cfar_semantics():
    """RTL-compat CFAR restatements (os_cfar.vhd:132, os_cfar_2d.vhd:189-213): 17-bit cells,
    the 1-D threshold wraps mod 2^17, the 2-D mean is floor(sum / 128) and its 17-bit bracket
    add wraps, threshold at full width."""
    # 1-D: a CUT of 30000 between refs of 40000 detects only because 4 * 40000 wraps to 28928
    m = np.full((1, 64), 40000.0)
    m[0, 20] = 30000.0
    det, thr = O.cfar_os1d_rtl(m, O.Cfar1D())
    assert det[0, 20] and thr[0, 20] == (4 * 40000) % (1 << 17) == 28928
    assert not O.cfar_os1d(m.astype(np.float32), O.Cfar1D())[0][0, 20]
    # quantisation: negatives -> 0, fractions floored, saturation at 2^17 - 1
    np.testing.assert_array_equal(O.q17(np.array([-3.0, 2.9, 2.0 ** 20])), [0, 2, (1 << 17) - 1])
    # 2-D: integer cells give the float definition's result wherever the brackets agree; the
    # tb_os_cfar_2d map (integers) finds both targets in compat arithmetic too
    z = np.load(GOLDEN / "tb_cfar2d.npz")
    rr, gr, rd, gd = z["params"].tolist()
    p = O.Cfar2D(ref_range=rr, guard_range=gr, ref_doppler=rd, guard_doppler=gd)
    det, thr = O.cfar_os2d_rtl(z["map"], p)
    assert det[30, 16] and det[50, 8]
    # the 17-bit bracket add: mean 100000 -> hi = 150000 mod 2^17 = 18928 < ranked -> scale_max
    mm = np.full((16, 32), 100000.0)
    det, thr = O.cfar_os2d_rtl(mm, O.Cfar2D())
    assert thr[8, 0] == 100000 * 6
    det_f, thr_f = O.cfar_os2d(mm.astype(np.float32), O.Cfar2D())
    assert thr_f[8, 0] == 100000 * 4                  # the float spec has no wrap: scale_nom


def test_mti_spectrum_rtl():
    """FMCW_COMPAT_MTI restatement: spectrum rounded half-to-even and saturated to int16, then
    the saturating canceller (doppler_notch.vhd:67-93)."""
    x = np.array([[0.5, 1.5, 2.5, 40000.0, -40000.0, 3.0]]) + 0j
    y = O.mti_spectrum_rtl(x, 2)
    np.testing.assert_array_equal(y.real[0], [0, 2, 0, 32765, -32768, 32767])
    y3 = O.mti_spectrum_rtl(x, 3)
    np.testing.assert_array_equal(y3.real[0], [0, 2, -2, 32765, -32768, 32767])


def _sat_cubes():
    rng = np.random.default_rng(77)
    a = rng.integers(-32768, 32768, (2, 32, 64, 2)).astype(np.int16)          # full-scale noise, 2 rx
    b = np.zeros((1, 32, 64, 2), np.int16)                                    # chirps of alternating sign
    b[..., 0] = (1000 * np.where(np.arange(32) % 2 == 0, 1, -1))[None, :, None]
    b[..., 1] = rng.integers(-300, 300, (1, 32, 64))
    return a, b


# (cube, range_shift, mti_mode, q15_rtl, mti_rtl) -> (window, word) saturations, as saturation_counts
# returned them before word_clips was split out of it
_SAT_RECORDED = {
    (0, 3, 0, True, False): (2213, 673), (0, 3, 0, False, True): (0, 634),
    (0, 3, 2, True, False): (2580, 2114), (0, 3, 2, False, True): (0, 2001),
    (0, 3, 3, True, False): (2987, 3526), (0, 3, 3, False, True): (0, 3452),
    (0, 4, 2, True, False): (1746, 115), (0, 4, 3, False, True): (0, 1112),
    (0, 5, 3, True, True): (1556, 32), (0, 6, 3, True, False): (1223, 0), (0, 6, 3, False, False): (0, 0),
    (1, 0, 0, True, False): (48, 33), (1, 0, 0, False, True): (0, 32),
    (1, 0, 2, True, False): (48, 126), (1, 0, 2, False, True): (0, 63),
    (1, 0, 3, True, False): (48, 126), (1, 1, 2, True, False): (47, 63),
    (1, 1, 3, True, False): (48, 125), (1, 1, 3, False, True): (0, 31), (1, 1, 0, False, True): (0, 0),
}


def test_word_clips_by_hand():
    """word_clips on a row whose clips can be counted by hand: words 0, 2, 2, 32767, -32768, 3."""
    x = np.array([[0.5, 1.5, 2.5, 40000.0, -40000.0, 3.0]]) + 0j
    assert O.word_clips(x, 0, False) == O.WordClips(word=2)
    # 2-pulse: 32765, -65535, 32771; 3-pulse: 32765, -98300 (= -32768 - 2 x 32767 + 2), 65539 + 32767
    assert O.word_clips(x, 2, False) == O.WordClips(word=2, canceller=2)
    assert O.word_clips(x, 3, False) == O.WordClips(word=2, canceller=2)
    # the 6-point Q15 ROM is (2621, 13044, 29890), mirrored: the window's gain 2 c / 32768 on the
    # canceller's output 0, 2, 0, 32765, -32768, 32767 is 1.82 at chirp 3 (clips), 0.80 and 0.16 after
    n = O.word_clips(x, 2, True)
    assert (n.word, n.canceller, n.doppler_window, n.range_window) == (2, 2, 1, 0)
    assert n.window_saturations == 1 and n.word_saturations == 4
    # the window sees the canceller's clipped output: unclipped, chirp 4 (-65535 x 0.80) would clip too
    assert O.word_clips(x, 0, True).doppler_window == 1         # words 32767 at chirp 3 only


def test_saturation_counts_unchanged_by_the_split():
    """saturation_counts returns the recorded totals on two small cubes, and they are the sum of
    word_clips' separate counts on the same spectrum plus the range window's clips on the cube."""
    cubes = _sat_cubes()
    seen = [0, 0, 0, 0]
    for (k, shift, mti, q15, rtl), want in _SAT_RECORDED.items():
        cube = cubes[k]
        assert O.saturation_counts(cube, shift, mti, q15, rtl) == want, (k, shift, mti, q15, rtl)
        if not (q15 or rtl):
            continue
        x = O.window_q15_cube(cube) if q15 else cube[..., 0].astype(np.float64) + 1j * cube[..., 1]
        spec = O.range_ct(x, window=False) * 2.0 ** -shift
        n = O.word_clips(spec, mti, q15)
        assert n.range_window == 0 and (mti or n.canceller == 0) and (q15 or n.doppler_window == 0)
        rw = O.range_window_clips(cube) if q15 else 0
        assert (rw + n.doppler_window, n.word + n.canceller) == want
        seen = [s + v for s, v in zip(seen, (n.word, n.canceller, n.doppler_window, rw))]
    assert all(seen)            # every one of the four counts took part
