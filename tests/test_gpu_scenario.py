"""The whole chain on the sea-clutter scenario (libfmcw.so on gfx950 through the C-ABI).

Inputs and expected values come from tests/scenario_ref.py; tests/test_scenario_host.py pins that
side on the fp64 oracle without a GPU (no cell within 1e-4 of its threshold, the detection counts,
which scans find which target, the tracker's behaviour), so a failure here means the GPU.

test_process: rtl/src/tb_tactical.vhd's own stimulus and the range-bin-domain scenario through MTI
off / 2-pulse / 3-pulse and the float and the integer (RTL-compatible) datapath, all scans in one
call.  test_device_chain / test_two_streams: fmcw_enqueue -> PlotExtractor -> DeviceTwsTracker on
the 256 x 64 scene with nothing downloaded in between.
"""
import numpy as np
import pytest

import scenario_ref as S
from conftest import rel_err
from fmcw import TRACK_DTYPE, TwsTracker
from plots_ref import assert_plots_match
from gpu_support import GUARD, MAP_TOL, RTL, Chain, Hip, assert_matches, check_map, make_core, run_cfar_stage, run_range_ct

pytestmark = pytest.mark.gpu

CASES = [(s, m, p) for s in S.SCENES for m in S.MTI_MODES for p in S.PATHS]
CASE_IDS = [f"{s.id}-mti{m}-{p}" for s, m, p in CASES]
KEY = ["range", "doppler", "mag", "threshold"]


def same_output(a, b):
    assert a.rd_map.tobytes() == b.rd_map.tobytes()
    np.testing.assert_array_equal(a.dets, b.dets)
    assert (a.window_saturations, a.word_saturations) == (b.window_saturations, b.word_saturations)


@pytest.mark.parametrize("scene,mti,path", CASES, ids=CASE_IDS)
def test_process(gpu, scene, mti, path):
    """One process call over all scans.

    Map: per scan and per bin above 1e-3 of the scan's peak within MAP_TOL = 1e-4 of the fp64 oracle
    end to end (integer path: of the oracle's Doppler stage on the words of the GPU's own range
    spectrum, as test_gpu_parity's q15_rtl cases, and per scan within 1e-4 of the fp64 end to end);
    the worst fraction of the tolerance is printed.  Integer path: status words 2 / 3 equal
    O.saturation_counts.  Detections of the fused path and of fmcw_cfar: bit-identical to the
    oracle's CFAR on the GPU's own map.  Against the reference's list a cell may differ only where
    the reference lies within 1e-4 of its threshold (the host test shows it never does), at most 1 %
    of a scan's records.  One call per scan, and one call in chunks whose boundary falls inside the
    notch, give the same bytes.  The scenario's facts on the GPU's list equal the oracle's."""
    cubes, _ = S.scene_cubes(scene)
    cubes = np.ascontiguousarray(cubes)
    n = scene.n_scans
    host = S.reference(scene, mti, path)
    with make_core(scene, mti, path, n) as core:
        out = core.process(cubes)
        stage = run_cfar_stage(core, out.rd_map)
        spec = run_range_ct(core, cubes, n) if path == "int" else None
        singles = [core.process(cubes[f:f + 1]) for f in range(n)]
    assert out.rd_map.shape == (n, scene.ns, scene.nc)

    if path == "int":
        ref = np.stack([S.int_map_from_spectrum(spec[f], mti) for f in range(n)])
        e2e = max(rel_err(out.rd_map[f], host.maps[f]) for f in range(n))
    else:
        ref, e2e = host.maps, 0.0
    worst = e2e
    for f in range(n):
        big = ref[f] >= 1e-3 * ref[f].max()
        worst = max(worst, rel_err(out.rd_map[f], ref[f]),
                    float(np.max(np.abs(out.rd_map[f][big] - ref[f][big]) / ref[f][big])))
    print(f"{scene.id} mti{mti} {path}: map worst {worst / MAP_TOL:.3f} of MAP_TOL")
    assert e2e <= MAP_TOL
    check_map(out.rd_map, ref)

    if path == "int":
        sat = (out.window_saturations, out.word_saturations)
        print(f"{scene.id} mti{mti} {path}: status words 2, 3 = {sat}")
        assert sat == S.saturation_counts(scene, mti)

    want = S.dets_on(scene, out.rd_map, path)
    np.testing.assert_array_equal(out.dets, want)
    np.testing.assert_array_equal(stage, want)

    ref_dets = S.dets_on(scene, ref.astype(np.float32), path)
    hr = scene.cfar.ref_range + scene.cfar.guard_range
    cell = lambda d: set(zip(d["frame"].tolist(), d["range"].tolist(), d["doppler"].tolist()))  # noqa: E731
    differ = cell(out.dets) ^ cell(ref_dets)
    print(f"{scene.id} mti{mti} {path}: {len(out.dets)} detections, {len(differ)} cells differ from the reference's list")
    for f in range(n):
        mine = [(r, d) for (ff, r, d) in differ if ff == f]
        if mine:
            near = S.near_threshold(scene, ref[f], path)
            assert all(near[r - hr, d] for r, d in mine), (f, mine)
            assert len(mine) <= 0.01 * int((ref_dets["frame"] == f).sum()), (f, mine)
    if scene.gen == "sea":
        assert min(int((out.dets["frame"] == f).sum()) for f in range(n)) >= 10

    for f in range(n):
        assert singles[f].rd_map.tobytes() == out.rd_map[f:f + 1].tobytes(), f
        np.testing.assert_array_equal(singles[f].dets[KEY], out.dets[out.dets["frame"] == f][KEY], err_msg=str(f))
    chunk = n // 2                 # 9 scans: 4 + 4 + 1, 5 scans: 2 + 2 + 1 -- a boundary between two notch scans
    assert chunk in scene.notch and chunk - 1 in scene.notch
    with make_core(scene, mti, path, n, chunk_frames=chunk) as core:
        assert core.info("chunk") == chunk
        same_output(core.process(cubes), out)

    assert S.facts(scene, out.dets, out.rd_map, path) == S.facts(scene, host.dets, host.maps.astype(np.float32), path)


# ---- the device chain (gpu_support.Chain) ----------------------------------------------------
def verify(scene, res, n_streams, rtl, oracles=None, hosts=None):
    """One chain result against the references, each on the GPU's own previous stage: detections =
    the oracle's CFAR on the GPU's map, plots = plots_ref on the GPU's detections, tracks = tws_dev_ref
    on the GPU's plots and the host TwsTracker fed the same plots scan by scan.  Returns the oracles'
    per-scan output and the carried (oracles, hosts)."""
    np.testing.assert_array_equal(res["dets"], S.dets_on(scene, res["map"], "float"))
    assert_plots_match(res["plots"], S.oracle_plots(scene, res["dets"]))
    groups = len(res["counts"])
    want, status, oracles = S.run_tracks(res["plots"], groups // n_streams, rtl, n_streams, oracles)
    guard = np.full(2, GUARD, np.uint32)           # (the counts buffer's own guard is Guarded's)
    assert_matches((res["status"], res["counts"], res["raw"], guard), want, status, n_streams, S.TRACK_CAP)
    assert status == [0, 0]
    hosts = hosts or [TwsTracker(INIT_HITS=S.TWS["init_hits"], COAST_MAX=S.TWS["coast_max"], rtl_compat=rtl)
                      for _ in range(n_streams)]
    for m in range(groups):
        h = hosts[m % n_streams]
        t = h.scan(res["plots"][res["plots"]["frame"] == m])
        assert (int(res["counts"][m, 0]), int(res["counts"][m, 1])) == (len(t), h.active_tracks), m
        assert res["raw"][m, :len(t) * 28].tobytes() == t.tobytes(), m
    return want, oracles, hosts


def gpu_tracks(res, n_streams, stream=0):
    """The GPU's track records in the shape scenario_ref.coasting_confirmed_track reads."""
    out = []
    for m in range(stream, len(res["counts"]), n_streams):
        t = res["raw"][m, :int(res["counts"][m, 0]) * 28].view(TRACK_DTYPE)
        out.append({stream: (t, int(res["counts"][m, 1]))})
    return out


def same_tracks(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in ("counts", "raw", "status"))


@RTL
def test_device_chain(gpu, rtl):
    """The 256 x 64 scene behind the 2-pulse canceller, 9 scans, one stream of the tracker.  One call
    of the three stages over all scans is verified stage by stage (verify) and confirms a track that
    later coasts (fact (d)); 4 + 5 scans in two calls give the same tracks (the track file stays on
    the device); the same holds for a second seed's cubes, and the chain captured into a graph and
    replayed on the second seed's cubes, then on the first's, gives each one's eager bytes."""
    sc, hip = S.CHAIN_SCENE, Hip()
    n = sc.n_scans
    cubes = [np.ascontiguousarray(S.scene_cubes(sc, seed)[0]) for seed in (None, S.CHAIN_SEED_2)]
    ch = Chain(hip, sc, n, 1, rtl)
    try:
        eager = []
        for cube in cubes:
            ch.cube.upload(cube)
            ch.trk.reset(stream=ch.stream.value)
            ch.clear()
            ch.enqueue()
            res = ch.result()
            verify(sc, res, 1, rtl)
            eager.append(res)
        assert S.coasting_confirmed_track(gpu_tracks(eager[0], 1))
        assert not same_tracks(eager[0], eager[1])

        # 4 + 5: frames restart at 0 in the second call, the track file carries on
        ch.cube.upload(cubes[0])
        ch.trk.reset(stream=ch.stream.value)
        ch.clear()
        ch.enqueue(0, 4)
        a = ch.result(4)
        _, oracles, hosts = verify(sc, a, 1, rtl)
        ch.clear()
        ch.enqueue(4, 5)
        b = ch.result(5)
        verify(sc, b, 1, rtl, oracles, hosts)
        assert np.concatenate([a["counts"], b["counts"]]).tobytes() == eager[0]["counts"].tobytes()
        assert np.concatenate([a["raw"], b["raw"]]).tobytes() == eager[0]["raw"].tobytes()
        assert np.concatenate([a["map"], b["map"]]).tobytes() == eager[0]["map"].tobytes()

        with hip.graph(lambda s: ch.enqueue(), ch.stream) as (exe, _):
            for k in (1, 0):
                ch.cube.upload(cubes[k])
                ch.trk.reset(stream=ch.stream.value)
                ch.clear()
                hip.replay(exe, ch.stream)
                got = ch.result()
                assert same_tracks(got, eager[k]), k
                np.testing.assert_array_equal(got["dets"], eager[k]["dets"])
                assert got["plots"].tobytes() == eager[k]["plots"].tobytes() and got["map"].tobytes() == eager[k]["map"].tobytes()
    finally:
        ch.close()


@RTL
def test_two_streams(gpu, rtl):
    """Two seeds as the two streams of one tracker: frame m is scan m // 2 of stream m % 2.  The oracle
    gives no scan without detections, so scan 4 of stream 1 is a zero cube (an empty list: the
    stream's tracks coast).  Each stream's tracks equal that seed's one-stream oracle."""
    sc, hip = S.CHAIN_SCENE, Hip()
    n = sc.n_scans
    a, b = (np.ascontiguousarray(S.scene_cubes(sc, seed)[0]) for seed in (None, S.CHAIN_SEED_2))
    b = b.copy()
    b[4] = 0
    cube = np.ascontiguousarray(np.stack([a, b], axis=1).reshape((2 * n,) + a.shape[1:]))
    assert cube[2].tobytes() == a[1].tobytes() and cube[9].tobytes() == b[4].tobytes()
    ch = Chain(hip, sc, 2 * n, 2, rtl)
    try:
        ch.cube.upload(cube)
        ch.clear()
        ch.enqueue()
        res = ch.result()
        want, _, _ = verify(sc, res, 2, rtl)
        assert not np.any(res["plots"]["frame"] == 9) and np.any(res["plots"]["frame"] == 8)
        for s in (0, 1):
            assert S.coasting_confirmed_track(gpu_tracks(res, 2, s), s)
        # stream 0 saw exactly the first seed's scans: the one-stream oracle on its plots
        mine = res["plots"][res["plots"]["frame"] % 2 == 0]
        solo, _, _ = S.run_tracks(S.as_records(mine, mine["frame"] // 2), n, rtl)
        assert [row[0] for row in want] == [row[0] for row in solo]
    finally:
        ch.close()
