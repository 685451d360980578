"""The sea-clutter scenario's cases and their reference side (fp64 oracle), shared by
test_scenario_host.py (which pins every fact here without a GPU) and test_gpu_scenario.py (which
holds the GPU to them).  A helper, not a test module.  TEST INFRASTRUCTURE ONLY.

Cases: rtl/src/tb_tactical.vhd's own QUICK_MODE stimulus (synth.tb_tactical_scans) and the same
scenario built in the range-bin domain (synth.sea_scenario), each through MTI off / 2-pulse /
3-pulse and through the float and the integer (RTL-compatible) datapath:

  float    Hamming windows, fp32 spectrum, |X|, 2-D OS-CFAR in fp32;
  int      window "q15_rtl" (integer windows on both axes), the canceller on the spectrum's 16-bit
           words (FMCW_COMPAT_MTI), range_shift INT_SHIFT so that nothing clips, |X|, the 17-bit
           integer 2-D CFAR (FMCW_COMPAT_CFAR).

Everything a GPU test compares against is computed here once per case and cached; callers must
not modify what they get.
"""
import functools
from dataclasses import dataclass

import numpy as np

import fmcw_oracle as O
import tws_dev_ref as R
from fmcw import synth
from plots_ref import plots_ref

MAP_TOL = 1e-4            # BASELINE.json north star (gpu_support.MAP_TOL)
NEAR = 1e-4               # a cell this close (relative) to its threshold may be decided either way
MTI_MODES = (0, 2, 3)
PATHS = ("float", "int")
QUICK_CFAR = dict(CFAR_REF_R=2, CFAR_REF_D=2, CFAR_GUARD_R=1, CFAR_GUARD_D=1)   # tb_tactical.vhd:37-40
DEFAULT_CFAR = dict(CFAR_REF_R=4, CFAR_REF_D=4, CFAR_GUARD_R=2, CFAR_GUARD_D=1)  # radar_core.vhd:12-19


@dataclass(frozen=True)
class Scene:
    id: str
    gen: str               # "tac": synth.tb_tactical_scans, "sea": synth.sea_scenario
    ns: int
    nc: int
    n_scans: int
    seed: int = 0
    quick: bool = True     # the QUICK_MODE CFAR generics, else the default window

    @property
    def generics(self):
        return QUICK_CFAR if self.quick else DEFAULT_CFAR

    @property
    def cfar(self):
        """The oracle's parameters for these generics (RadarCore's mapping: the RTL's *_R generics
        act along Doppler, the *_D ones along range)."""
        g = self.generics
        return O.Cfar2D(ref_range=g["CFAR_REF_D"], guard_range=g["CFAR_GUARD_D"],
                        ref_doppler=g["CFAR_REF_R"], guard_doppler=g["CFAR_GUARD_R"])

    @property
    def notch(self):
        """0-based scans in which the fighters fly the notch."""
        k = self.n_scans // 2
        return tuple(range(k - 1, min(k + 2, self.n_scans)))


SCENES = (
    Scene("tac-128x32", "tac", 128, 32, 5),
    Scene("sea-128x32", "sea", 128, 32, 9, seed=1),
    Scene("sea-256x64", "sea", 256, 64, 9, seed=105, quick=False),
)
BY_ID = {s.id: s for s in SCENES}
CHAIN_SCENE = BY_ID["sea-256x64"]
CHAIN_SEED_2 = 3           # the second seed of the device-chain tests (graph replay, second stream)

# range_shift of the integer datapath, (scene, canceller): the smallest at which the fp64 oracle
# clips nowhere (test_scenario_host.test_integer_shift_is_the_smallest_clean_one)
INT_SHIFT = {
    ("tac-128x32", 0): 0, ("tac-128x32", 2): 0, ("tac-128x32", 3): 1,
    ("sea-128x32", 0): 5, ("sea-128x32", 2): 5, ("sea-128x32", 3): 6,
    ("sea-256x64", 0): 6, ("sea-256x64", 2): 6, ("sea-256x64", 3): 7,
}

# the trackers' generics of the device-chain tests: within the ranges test_gpu_tws_dev.py uses
# (init_hits 0..2, coast_max 0..5, the default gates)
TWS = dict(init_hits=2, coast_max=3)
PLOT_WIN = (1, 1)
PLOT_CAP = 1024
TRACK_CAP = 32


def to_complex(cube_i16):
    x = np.asarray(cube_i16).astype(np.float64)
    return x[..., 0] + 1j * x[..., 1]


@functools.lru_cache(maxsize=None)
def scene_cubes(scene: Scene, seed=None):
    """(int16 cubes [scan][1][chirp][sample][2], truth) of a scene (seed: another sea_scenario seed)."""
    if scene.gen == "tac":
        cubes, truth = synth.tb_tactical_scans(scene.n_scans, quick=True)
    else:
        cubes, truth = synth.sea_scenario(scene.ns, scene.nc, scene.n_scans, scene.seed if seed is None else seed)
    assert cubes.shape == (scene.n_scans, 1, scene.nc, scene.ns, 2)
    cubes.setflags(write=False)
    return cubes, truth


def oracle_map(scene: Scene, cube, mti: int, path: str):
    """The fp64 end-to-end map [range][doppler] of one scan's cube [1][chirp][sample][2]."""
    if path == "int":
        return O.process(cube, None, mti_mode=mti, q15_rtl=True, mti_rtl=True,
                         range_shift=INT_SHIFT[scene.id, mti])["mag"]
    return O.process(to_complex(cube), None, mti_mode=mti)["mag"]


def int_map_from_spectrum(spec, mti: int):
    """The integer datapath's fp64 map from a scaled range spectrum [1][range][chirp] (the GPU's own
    fp32 one: a word then rounds the same on both sides, as in test_gpu_parity's q15_rtl cases)."""
    rd = O.doppler_stage(np.asarray(spec).astype(np.complex128), mti_mode=mti, q15_rtl=True, mti_rtl=True)
    return O.magnitude(rd, rx_axis=0)


def cfar_on(scene: Scene, mag32, path: str):
    """(det mask, threshold) of the oracle's 2-D CFAR on one float32 map."""
    fn = O.cfar_os2d_rtl if path == "int" else O.cfar_os2d
    return fn(np.asarray(mag32, np.float32), scene.cfar)


def dets_on(scene: Scene, maps32, path: str):
    """The oracle's detection records (O.DET_DTYPE) on float32 maps [scan][range][doppler]."""
    out = []
    for f in range(len(maps32)):
        det, thr = cfar_on(scene, maps32[f], path)
        rec = O.detections_rtl if path == "int" else O.detections
        out.append(rec(det, np.asarray(maps32[f], np.float32), thr, frame=f))
    return np.concatenate(out)


def near_threshold(scene: Scene, mag64, path: str):
    """Tested cells of an fp64 map within NEAR (relative) of the CFAR's decision: cut == threshold
    in the float path; in the integer path the cut's word exceeds T from T + 1 on."""
    det, thr = cfar_on(scene, mag64.astype(np.float32), path)
    hr = scene.cfar.ref_range + scene.cfar.guard_range
    rows = slice(hr, mag64.shape[0] - hr)
    edge = thr[rows].astype(np.float64) + (1.0 if path == "int" else 0.0)
    return np.abs(mag64[rows] - edge) <= NEAR * np.maximum(edge, 1e-30)


@dataclass(frozen=True)
class Reference:
    maps: np.ndarray        # [scan][range][doppler] fp64, the end-to-end oracle
    dets: np.ndarray        # O.DET_DTYPE, the oracle CFAR on maps.astype(float32)
    n_near: int             # cells within NEAR of their threshold, all scans
    counts: tuple           # detections per scan


@functools.lru_cache(maxsize=None)
def reference(scene: Scene, mti: int, path: str, seed=None) -> Reference:
    cubes, _ = scene_cubes(scene, seed)
    maps = np.stack([oracle_map(scene, cubes[f], mti, path) for f in range(scene.n_scans)])
    maps.setflags(write=False)
    dets = dets_on(scene, maps.astype(np.float32), path)
    dets.setflags(write=False)
    n_near = int(sum(near_threshold(scene, maps[f], path).sum() for f in range(scene.n_scans)))
    return Reference(maps, dets, n_near, tuple(int((dets["frame"] == f).sum()) for f in range(scene.n_scans)))


def saturation_counts(scene: Scene, mti: int, seed=None):
    """(status word 2, status word 3) of the integer datapath over all scans: O.saturation_counts."""
    cubes, _ = scene_cubes(scene, seed)
    per = [O.saturation_counts(cubes[f], INT_SHIFT[scene.id, mti], mti, q15_rtl=True, mti_rtl=True)
           for f in range(scene.n_scans)]
    return sum(p[0] for p in per), sum(p[1] for p in per)


# ---- what the scenario is about --------------------------------------------------------------
def found(scene: Scene, dets, truth):
    """found[scan][target]: a detection within one bin (Doppler circular) of the target's truth."""
    out = []
    for f, bins in enumerate(truth):
        d = dets[dets["frame"] == f]
        r, dp = d["range"].astype(np.int64), d["doppler"].astype(np.int64)
        row = []
        for rb, db in bins:
            dd = np.abs(dp - db)
            row.append(bool(np.any((np.abs(r - rb) <= 1) & (np.minimum(dd, scene.nc - dd) <= 1))))
        out.append(tuple(row))
    return tuple(out)


def scale_at(scene: Scene, mag32, path: str, r: int, d: int) -> int:
    """The scale bracket (scale_min / scale_nom / scale_max) the CFAR applied at a tested cell."""
    m = np.asarray(mag32, np.float32)
    if path == "int":
        m = O.q17(m).astype(np.float32)
    p = scene.cfar
    refs = np.sort(np.array([m[r + dr, (d + dd) % scene.nc] for dr, dd in O.cfar2d_offsets(p)], np.float32))
    _, thr = cfar_on(scene, mag32, path)
    return int(round(float(thr[r, d]) / float(refs[p.rank]))) if refs[p.rank] > 0 else 0


def facts(scene: Scene, dets, maps32, path: str, seed=None):
    """The scenario's facts on a detection list and the maps it came from: which scans find each
    target, and for the low flyer of a sea scene the scale bracket at its cell."""
    _, truth = scene_cubes(scene, seed)
    out = {"found": found(scene, dets, truth)}
    if scene.gen == "sea":
        out["low_flyer_scale"] = tuple(scale_at(scene, maps32[f], path, *truth[f][-1]) for f in range(scene.n_scans))
    return out


# ---- plots and tracks ------------------------------------------------------------------------
def as_records(plots, frames=None):
    """plots_ref's records as an O.DET_DTYPE list (what a tracker reads of a plot)."""
    out = np.zeros(len(plots), O.DET_DTYPE)
    for k in ("frame", "range", "doppler", "mag", "threshold"):
        out[k] = plots[k]
    if frames is not None:
        out["frame"] = frames
    return out


def oracle_plots(scene: Scene, dets):
    return plots_ref(dets, scene.ns, scene.nc, *PLOT_WIN)


def run_tracks(records, n_scans, rtl, n_streams=1, oracles=None):
    """tws_dev_ref.run_ref with this module's generics: (out[scan][stream], status, oracles)."""
    oracles = oracles or R.make_oracles(n_streams, rtl, **TWS)
    out, status = R.run_ref(records, n_scans, n_streams, oracles)
    return out, status, oracles


def coasting_confirmed_track(out, stream=0):
    """Fact (d): some track id is reported FIRM in one scan and COAST in a later one.  Returns the
    ids for which that holds."""
    firm, ok = set(), set()
    for row in out:
        tracks, _ = row[stream]
        for t in tracks:
            if int(t["status"]) == 2:
                firm.add(int(t["id"]))
            elif int(t["status"]) == 3 and int(t["id"]) in firm:
                ok.add(int(t["id"]))
    return ok
