"""The sea-clutter scenario without a GPU: the two generators of fmcw.synth against what
rtl/src/tb_tactical.vhd says, and the reference side of every assertion of test_gpu_scenario.py
(tests/scenario_ref.py) pinned on the fp64 oracle, so that a GPU failure can only mean the GPU.

(a) no cell of any scan within 1e-4 of its threshold in the fp64 end-to-end map; (b) detection
counts; (c) which scans find which target with MTI off / 2-pulse / 3-pulse, and the low flyer;
(d) the tracker confirms a track and coasts it; (e) the C backend on the 128 x 32 case it can run.
"""
import numpy as np
import pytest

import cpu_backend as CB
import fmcw_oracle as O
import scenario_ref as S
from conftest import rel_err
from fmcw import synth

CASES = [(s, m, p) for s in S.SCENES for m in S.MTI_MODES for p in S.PATHS]
CASE_IDS = [f"{s.id}-mti{m}-{p}" for s, m, p in CASES]
SEA = [s for s in S.SCENES if s.gen == "sea"]


# ---- the generators against the testbench's text ---------------------------------------------
def test_tactical_first_draws_are_ieee_uniform():
    """Chirp 0, samples 0 and 1 of scan 1 hold no target (the bins are 89 and 77), so they are clutter
    plus noise from draws 0..7 of UNIFORM(42, 42): amplitude, phase, u1, u2 per sample.  The stream
    runs on: the first sample of scan 2 takes draws 16384..16387."""
    cubes, _ = S.scene_cubes(S.BY_ID["tac-128x32"])
    u, _, _ = synth.ieee_uniform(42, 42, 128 * 32 * 4 + 4)

    def sample(d, s, c):
        amp = 200.0 * (1.0 - s / 128.0) * d[0]
        ph = 2.0 * np.pi * (s * s / 1280.0 + (d[1] - 0.5) * 4.0 * c / 32.0)
        g = np.sqrt(-2.0 * np.log(max(d[2], 1e-10)))
        z = amp * np.exp(1j * ph) + 50.0 * g * np.exp(2j * np.pi * d[3])
        return [int(np.sign(v) * np.floor(abs(v) + 0.5)) for v in (z.real, z.imag)]
    assert cubes[0, 0, 0, 0].tolist() == sample(u[0:4], 0, 0)
    assert cubes[0, 0, 0, 1].tolist() == sample(u[4:8], 1, 0)
    assert cubes[0, 0, 1, 0].tolist() == sample(u[512:516], 0, 1)
    assert cubes[1, 0, 0, 0].tolist() == sample(u[16384:16388], 0, 0)


def test_tactical_bins_follow_the_testbench():
    """vel_to_doppler_bin (integer() of 2 v / 0.1 / prf x 32, plus N / 2, wrapped) over the stagger:
    fighters 21 / 24 / 26 and the attacker 30 / 0 / 2 at 8 / 9 / 10 kHz -- bin 0 at 9 kHz is the
    blind speed the stagger exists for; bin 16 for the fighters in the notch; range bins
    integer(range / 120000 x 128) of the testbench's kinematics."""
    _, truth = synth.tb_tactical_scans(9)                 # notch at scans 4, 5, 6
    want_f, want_a = (21, 24, 26), (30, 0, 2)
    r_f, r_a = [45 * 1852.0, 45 * 1852.0 - 50.0], 39 * 1852.0
    for k, bins in enumerate(truth):
        notch = k + 1 in (4, 5, 6)
        r_f = [r - (0.0 if notch else 340.29) * 0.5 for r in r_f]
        r_a -= 0.65 * 340.29 * 0.5
        assert [d for _, d in bins] == [16 if notch else want_f[k % 3]] * 2 + [want_a[k % 3]], k
        assert [r for r, _ in bins] == [int(np.floor(r / 120000.0 * 128 + 0.5)) for r in r_f + [r_a]], k
    # the 5-scan QUICK_MODE run: NOTCH_SCAN = 2
    _, quick = S.scene_cubes(S.BY_ID["tac-128x32"])
    assert [b[0][1] for b in quick] == [21, 16, 16, 16, 24] and [b[2][1] for b in quick] == [30, 0, 2, 30, 0]
    assert S.BY_ID["tac-128x32"].notch == (1, 2, 3) and S.BY_ID["sea-128x32"].notch == (3, 4, 5)


def test_tactical_target_is_a_gated_pulse():
    """A target adds to the five fast-time samples within 2 of its range bin only (the testbench
    gates on the sample index): the noise-free difference between two runs is not available, so
    compare the energy there with the rest of the chirp."""
    cubes, truth = S.scene_cubes(S.BY_ID["tac-128x32"])
    x = S.to_complex(cubes[0, 0])
    rb = truth[0][2][0]                                    # the attacker: 1720 counts
    assert np.abs(x[:, rb]).mean() > 1000 and np.abs(x[:, rb + 3:rb + 8]).mean() < 200


@pytest.mark.parametrize("scene", S.SCENES, ids=lambda s: s.id)
def test_no_sample_is_clipped(scene):
    cubes, _ = S.scene_cubes(scene)
    assert cubes.dtype == np.int16 and np.abs(cubes.astype(np.int32)).max() < 32000


def test_sea_clutter_stops_at_the_edge():
    """The clutter's range spectrum is zero at and beyond the edge, to rounding, and carries the level
    200 (1 - r / n_range) below it."""
    ns, nc = 192, 48
    edge = synth.sea_clutter_edge(ns)
    assert edge == 32 and synth.sea_clutter_edge(128) == 21 and synth.sea_clutter_edge(256) == 43
    x = synth.sea_clutter(np.random.default_rng(5), ns, nc)
    spec = np.fft.fft(x, axis=-1) / ns                      # [chirp][range bin] = level x g
    assert np.abs(spec[:, edge:]).max() <= 1e-12 * np.abs(spec).max()
    rms = np.sqrt((np.abs(spec[:, :edge]) ** 2).mean(axis=0))
    level = 200.0 * (1.0 - np.arange(edge) / ns)
    # 48 correlated chirps: about 48 (1 - rho) / (1 + rho) = 2.5 independent looks per bin
    assert 0.5 < np.median(rms / level) < 1.5


def test_sea_clutter_lag_one_correlation():
    """rho = 0.9 from chirp to chirp.  256 independent range bins x 63 pairs; Bartlett's variance of the
    lag-1 estimate of an AR(1) series, (1 - rho^2) / n, gives sd = sqrt(0.19 / 16128) = 0.0034: held
    to 4 sd."""
    ns, nc = 1536, 64
    x = synth.sea_clutter(np.random.default_rng(6), ns, nc)
    g = (np.fft.fft(x, axis=-1) / ns)[:, :synth.sea_clutter_edge(ns)]
    g = g / (200.0 * (1.0 - np.arange(g.shape[1]) / ns))
    r1 = (g[1:] * np.conj(g[:-1])).mean() / (np.abs(g) ** 2).mean()
    assert abs(r1.real - 0.9) <= 4 * 0.0034 and abs(r1.imag) <= 4 * 0.0034
    assert abs((np.abs(g) ** 2).mean() - 1.0) <= 0.05        # unit variance (about 1,700 independent looks)


def test_sea_targets_are_tones_at_the_stated_bins():
    """The oracle's map of scan 1 peaks, beyond the clutter, at the truth bin of the two fighters (one
    tone each at fractional range bin 88.7, 50 m apart: they add up) and next at the attacker's;
    Doppler without the testbench's N / 2 offset: (2 v / 0.1 / 8000 x 32) mod 32 = 4.8 and 14.3."""
    sc = S.BY_ID["sea-128x32"]
    _, truth = S.scene_cubes(sc)
    assert truth[0][:3] == [(89, 5), (89, 5), (77, 14)] and truth[0][3] == (21 // 2, 27)
    assert [b[0][1] for b in truth] == [5, 8, 10, 0, 0, 0, 5, 8, 10]
    m = S.reference(sc, 0, "float").maps[0]
    beyond = m[21 + 4:].copy()                             # beyond the clutter and its window skirt
    r, d = np.unravel_index(np.argmax(beyond), beyond.shape)
    assert (r + 25, d) == (89, 5)
    beyond[r - 3:r + 4] = 0
    r, d = np.unravel_index(np.argmax(beyond), beyond.shape)
    assert (r + 25, d) == (77, 14)


# ---- the reference side of the GPU tests ------------------------------------------------------
@pytest.mark.parametrize("scene,mti,path", CASES, ids=CASE_IDS)
def test_reference_has_no_cell_near_its_threshold(scene, mti, path):
    """(a), and (b): at least 10 detections per scan of a sea scene, 0 to 3 on the testbench's own
    stimulus (targets and clutter are white in range there), all far below the list's capacity."""
    ref = S.reference(scene, mti, path)
    assert ref.n_near == 0
    if scene.gen == "sea":
        assert min(ref.counts) >= 10 and max(ref.counts) <= 300
    else:
        assert max(ref.counts) <= 3


@pytest.mark.parametrize("scene", S.SCENES, ids=lambda s: s.id)
def test_integer_shift_is_the_smallest_clean_one(scene):
    for mti in S.MTI_MODES:
        sh = S.INT_SHIFT[scene.id, mti]
        assert S.saturation_counts(scene, mti) == (0, 0)
        if sh:
            cubes, _ = S.scene_cubes(scene)
            assert any(O.saturation_counts(cubes[f], sh - 1, mti, q15_rtl=True, mti_rtl=True) != (0, 0)
                       for f in range(scene.n_scans)), (scene.id, mti)


@pytest.mark.parametrize("scene", SEA, ids=lambda s: s.id)
@pytest.mark.parametrize("path", S.PATHS)
def test_scenario_facts(scene, path):
    """(c) on the oracle's lists: every fighter and the attacker are found outside the notch by every
    canceller; in the notch (Doppler 0) the fighters are found with MTI off and lost behind the
    3-pulse canceller; the attacker is found in every scan; the low flyer is found in every scan
    behind the 2-pulse canceller and missed in at least one with MTI off."""
    f = {}
    for mti in S.MTI_MODES:
        ref = S.reference(scene, mti, path)
        f[mti] = S.facts(scene, ref.dets, ref.maps.astype(np.float32), path)
    for mti in S.MTI_MODES:
        for k, row in enumerate(f[mti]["found"]):
            assert row[2], (mti, k)
            if k not in scene.notch:
                assert row[0] and row[1], (mti, k)
    for k in scene.notch:
        assert f[0]["found"][k][:2] == (True, True) and f[3]["found"][k][:2] == (False, False)
    assert all(row[3] for row in f[2]["found"])
    assert not all(row[3] for row in f[0]["found"])
    for mti in S.MTI_MODES:
        assert set(f[mti]["low_flyer_scale"]) <= {2, 4, 6}


def test_fp32_rounding_alone_is_within_the_tolerance():
    """What fp32 costs against fp64 on this input, without any kernel: the float path in complex64
    NumPy (fp32 windows, FFTs, canceller and magnitude) against the oracle, per scan and per bin
    above 1e-3 of the scan's peak.  Printed as a fraction of MAP_TOL."""
    for scene in S.SCENES:
        cubes, _ = S.scene_cubes(scene)
        for mti in S.MTI_MODES:
            ref = S.reference(scene, mti, "float").maps
            worst = 0.0
            for f in range(scene.n_scans):
                x = (cubes[f, 0, ..., 0] + 1j * cubes[f, 0, ..., 1].astype(np.float32)).astype(np.complex64)
                spec = np.fft.fft(x * O.window_f32(scene.ns), axis=-1).T.astype(np.complex64)
                spec = O.mti(spec, mti).astype(np.complex64)
                rd = np.fft.fft(spec * O.window_f32(scene.nc), axis=-1).astype(np.complex64)
                assert rd.dtype == np.complex64
                got = np.abs(rd)
                big = ref[f] >= 1e-3 * ref[f].max()
                worst = max(worst, rel_err(got, ref[f]), float(np.max(np.abs(got[big] - ref[f][big]) / ref[f][big])))
            print(f"{scene.id} mti{mti}: fp32 NumPy vs fp64, worst {worst / S.MAP_TOL:.3f} of MAP_TOL")
            assert worst <= S.MAP_TOL


@pytest.mark.parametrize("rtl", [False, True])
@pytest.mark.parametrize("seed", [None, S.CHAIN_SEED_2])
def test_tracker_confirms_and_coasts(rtl, seed):
    """(d), and (b) for the device chain: over 9 scans the oracle's plots of the 256 x 64 scene with
    the 2-pulse canceller stay below the tracker's 64 detections per scan and the plot capacity, and
    tws_oracle confirms at least one track that coasts in a later scan."""
    sc = S.CHAIN_SCENE
    plots = S.oracle_plots(sc, S.reference(sc, 2, "float", seed).dets)
    per_scan = [int((plots["frame"] == f).sum()) for f in range(sc.n_scans)]
    assert 10 <= min(per_scan) and max(per_scan) < 64 and len(plots) < S.PLOT_CAP
    out, status, _ = S.run_tracks(S.as_records(plots), sc.n_scans, rtl)
    assert status == [0, 0]
    assert S.coasting_confirmed_track(out)
    assert max(len(row[0][0]) for row in out) <= S.TRACK_CAP


def test_c_backend_on_the_small_scene():
    """(e): oracle/fmcw_cpu.c runs the float path with MTI off (it has no canceller): the 128 x 32 sea
    scene through it, held to the checks the GPU gets -- map within its 1e-5 of the oracle, its CFAR
    bit-exact with the oracle's on its own map, the list equal to the reference's, the same facts."""
    sc = S.BY_ID["sea-128x32"]
    cubes, _ = S.scene_cubes(sc)
    ref = S.reference(sc, 0, "float")
    m, d, n = CB.process(S.to_complex(cubes).astype(np.complex64), sc.cfar, threads=4)
    assert n == len(d)
    for f in range(sc.n_scans):
        assert rel_err(m[f], ref.maps[f]) <= 1e-5
    np.testing.assert_array_equal(d, S.dets_on(sc, m, "float"))
    key = ["frame", "range", "doppler"]
    np.testing.assert_array_equal(d[key], ref.dets[key])
    assert S.facts(sc, d, m, "float") == S.facts(sc, ref.dets, ref.maps.astype(np.float32), "float")
