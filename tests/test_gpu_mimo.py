"""The TDM-MIMO virtual array on the GPU (fmcw_mimo_* of libfmcw.so on gfx950 through the C-ABI), every
case against tests/mimo_ref.py (the specification in fp64 NumPy).  The tolerance is
mimo_ref.assert_rows_match's (1e-4 of each output row's maximum); every comparison prints the worst
fraction of the bound used.  "none" is held to the input's bytes.

Shapes: n_range 64, 3 frames, every (n_tx, n_d) of n_tx 2, 4, 8 x n_d 32 .. 512 up to 1024 chirps (each n_d
its own kernel instantiation: 2 .. 32 lanes per sequence, 32 .. 2 sequences and 16 .. 1 input rows per
wave tile), n_rx 1 and 3 (3: the frame / channel split of a tile's row is no shift), and the header's
limits.  The input is mimo_ref.full_scale_case, a white Gaussian spectrum from the host: every output cell
has the scale of its row, so a misplaced, stale or never-stored cell is out of bound wherever it falls
(tests/test_mimo_host.py measures it on the reference).  run() also fails on any output word that still
holds the sentinel the buffer was filled with, and on any byte written behind the output.
"""
import functools

import numpy as np
import pytest

from fmcw import DET_DTYPE, BeamFormer, BearingEstimator, DeviceBuffer, RadarCore, VirtualArray, steering_weights, synth
from fmcw import _lib as L
import mimo_ref as M
from bearings_ref import assert_bearings_match, bearings_ref
from gpu_support import SENTINEL, Hip, assert_all_written, assert_sentinel_after, range_ct_spectrum, sentinel_buffer

pytestmark = pytest.mark.gpu

TAIL = 4096       # sentinel bytes checked behind every output
NF, NR = M.FS_NF, M.FS_NR


def run(va, spec, n_frames=None):
    """One fmcw_mimo_enqueue on a host spectrum into a sentinel-filled buffer: the output, after checking
    that the TAIL bytes behind it kept the sentinel and that every word of it was written."""
    n_frames = len(spec) if n_frames is None else n_frames
    nbytes = n_frames * va.frame_bytes()
    dspec = DeviceBuffer(max(spec.nbytes, 16))
    dspec.upload(spec)
    do = sentinel_buffer(nbytes + TAIL)
    try:
        va.enqueue(dspec, n_frames, do)
        raw = do.download(np.uint8, (nbytes + TAIL,))
    finally:
        dspec.free()
        do.free()
    assert_sentinel_after(raw, nbytes, 1, "virtual array output")
    assert_all_written(raw[:nbytes], "virtual array output")
    return raw[:nbytes].view(np.complex64).reshape(n_frames, va.n_virtual, va.cfg.n_range, va.n_d).copy()


@functools.lru_cache(maxsize=None)
def case(n_tx, n_d, n_rx):
    """(spec, the fp64 reference, the raw de-interleave) of a full-scale case, computed once."""
    spec = M.full_scale_case(n_tx, n_d, n_rx)
    ref, raw = M.mimo_ref(spec, n_tx), M.mimo_ref(spec, n_tx, "none")
    for a in (ref, raw):
        a.setflags(write=False)
    return spec, ref, raw


def check_both(n_tx, n_d, n_rx):
    spec, ref, raw = case(n_tx, n_d, n_rx)
    label = f"{NR} x {n_tx * n_d} chirps, tx{n_tx} x rx{n_rx}, n_d {n_d}"
    with VirtualArray(NR, n_tx * n_d, n_rx, n_tx) as va:
        assert (va.n_virtual, va.n_d) == (n_tx * n_rx, n_d)
        got = run(va, spec)
    M.assert_rows_match(got, ref, label=label + " dft")
    with VirtualArray(NR, n_tx * n_d, n_rx, n_tx, align="none") as va:
        assert run(va, spec).tobytes() == raw.tobytes(), label + " none"
    return got


@pytest.mark.parametrize("n_rx", M.FS_RXS)
@pytest.mark.parametrize("n_tx,n_d", M.FS_MATRIX)
def test_matrix(gpu, n_tx, n_d, n_rx):
    """"dft" within the bound in every cell, "none" byte-exact; TX 0's channels are u_0 up to rounding."""
    got = check_both(n_tx, n_d, n_rx)
    spec, _, raw = case(n_tx, n_d, n_rx)
    M.assert_rows_match(got[:, :n_rx], raw[:, :n_rx], label="TX 0 against the copy")


@pytest.mark.parametrize("n_tx,n_d,n_rx", M.FS_LIMITS)
def test_limits(gpu, n_tx, n_d, n_rx):
    """32 transmitters (256-B output chunks, the smallest), 64 virtual channels of 32 receivers, and one
    transmitter at 1024 chirps, where both modes are the copy."""
    got = check_both(n_tx, n_d, n_rx)
    if n_tx == 1:
        assert got.tobytes() == case(n_tx, n_d, n_rx)[0].tobytes()


@pytest.mark.parametrize("n_tx,n_d", [(2, 32), (2, 512), (8, 128)])
@pytest.mark.parametrize("align", ["dft", "none"])
def test_grid_independence(gpu, n_tx, n_d, align):
    """1 and 3 workgroups through the hook, then the built-in grid again, at the smallest and the largest
    n_chirps (3 rx, 3 frames: 36 .. 576 wave tiles over 4 and 12 waves): a workgroup passes several tiles,
    channels and frames.  The reference's values, and the same bytes each time."""
    spec, ref, raw = case(n_tx, n_d, 3)
    with VirtualArray(NR, n_tx * n_d, 3, n_tx, align=align) as va:
        base = run(va, spec)
        for grid in (1, 3, 0):
            va.set_grid_for_test(grid)
            got = run(va, spec)
            if align == "dft":
                M.assert_rows_match(got, ref, label=f"tx{n_tx} x {n_d} grid {grid}")
            else:
                assert got.tobytes() == raw.tobytes(), grid
            assert got.tobytes() == base.tobytes(), grid


def test_fewer_frames_than_the_buffer(gpu):
    """n_frames = 2 of an uploaded 3: nothing is stored beyond two output frames."""
    spec, ref, _ = case(4, 64, 3)
    with VirtualArray(NR, 256, 3, 4) as va:
        got = run(va, spec, n_frames=2)
    M.assert_rows_match(got, ref[:2], label="two of three frames")


def test_zero_frames_and_bad_arguments_write_nothing(gpu):
    lib = L.load()
    with VirtualArray(NR, 64, 2, 2) as va:
        nbytes = va.frame_bytes()
        din = sentinel_buffer(nbytes)
        do = sentinel_buffer(nbytes + TAIL)
        try:
            va.enqueue(din, 0, do)
            assert lib.fmcw_mimo_enqueue(va._h, None, 0, None, None) == L.FMCW_OK      # nothing is looked at
            assert lib.fmcw_mimo_enqueue(va._h, None, 1, do.ptr, None) == L.FMCW_EINVAL
            assert lib.fmcw_mimo_enqueue(va._h, din.ptr, 1, None, None) == L.FMCW_EINVAL
            assert lib.fmcw_mimo_enqueue(va._h, din.ptr, 1, do.ptr + 8, None) == L.FMCW_EINVAL
            assert lib.fmcw_last_error() == b"out_dev must be 16-byte aligned"
            assert lib.fmcw_mimo_enqueue(va._h, din.ptr + 8, 1, do.ptr, None) == L.FMCW_EINVAL
            assert lib.fmcw_last_error() == b"spec_dev must be 16-byte aligned"
            for src, dst in ((0, 0), (0, 16), (16, 0), (0, nbytes - 16)):        # in place, and partial overlaps
                assert lib.fmcw_mimo_enqueue(va._h, do.ptr + src, 1, do.ptr + dst, None) == L.FMCW_EINVAL
                assert b"overlaps" in lib.fmcw_last_error()
            assert_sentinel_after(do.download(np.uint8, (nbytes + TAIL,)), what="the output of calls that must write nothing")
        finally:
            din.free()
            do.free()


def test_form(gpu):
    """form() on a host spectrum and on a device one gives enqueue's bytes."""
    spec, ref, _ = case(2, 64, 3)
    with VirtualArray(NR, 128, 3, 2) as va:
        got = run(va, spec)
        assert va.form(spec).tobytes() == got.tobytes()
        ds = DeviceBuffer(spec.nbytes)
        ds.upload(spec)
        try:
            assert va.form(ds).tobytes() == got.tobytes()
        finally:
            ds.free()
        with pytest.raises(ValueError, match="whole number of frames"):
            va.form(spec.reshape(-1)[:-2])


# ---- after fmcw_range_ct: the graph and the chain ----------------------------------------------------
CH_TX, CH_RX, CH_NC, CH_SEED, CH_NU = 2, 4, 128, 830, 0.2     # tests/test_mimo_host.py's first physics case


def chain_cube():
    cube = synth.tdm_frames(1, NR, CH_NC, CH_RX, CH_TX, "random_target", CH_SEED, CH_NU)
    (r, d, _), = synth._targets("random_target", NR, CH_NC, np.random.Generator(np.random.PCG64(CH_SEED)))[0]
    return cube, int(round(r)), int(round(d))


def test_graph_replay_after_range_ct(gpu):
    """fmcw_range_ct and fmcw_mimo_enqueue captured once into one graph and replayed twice, the output
    refilled with the sentinel in between: each replay writes the same bytes, the reference's values on
    the replay's own spectrum."""
    cube, _, _ = chain_cube()
    hip = Hip()
    with RadarCore(N_RANGE=NR, N_DOPPLER=CH_NC, N_RX=CH_RX, cfar="none", max_frames=1) as core, \
            VirtualArray(NR, CH_NC, CH_RX, CH_TX) as va:
        nbytes = va.frame_bytes()
        dc = DeviceBuffer(cube.nbytes)
        ds = DeviceBuffer(nbytes)
        do = sentinel_buffer(nbytes + TAIL)

        def calls(s):
            core.range_ct(dc, ds, 1, stream=s.value)
            va.enqueue(ds, 1, do, stream=s.value)
        try:
            dc.upload(cube)
            with hip.graph(calls) as (exe, s):
                seen = []
                for k in (0, 1):
                    do.upload(np.full(nbytes + TAIL, SENTINEL, np.uint8))
                    hip.replay(exe, s)
                    spec = ds.download(np.complex64, (1, CH_RX, NR, CH_NC))
                    raw = do.download(np.uint8, (nbytes + TAIL,))
                    assert_sentinel_after(raw, nbytes, 1, f"replay {k}")
                    assert_all_written(raw[:nbytes], f"replay {k}")
                    got = raw[:nbytes].view(np.complex64).reshape(1, CH_TX * CH_RX, NR, CH_NC // CH_TX)
                    M.assert_rows_match(got, M.mimo_ref(spec, CH_TX), label=f"replay {k}")
                    seen.append(raw.tobytes())
                assert seen[0] == seen[1]
        finally:
            for b in (dc, ds, do):
                b.free()


def test_chain_to_bearings_and_beams(gpu):
    """tdm_frames (2 TX x 4 RX, 64 x 128 chirps, a target 9.3 Doppler bins off zero at nu 0.2) ->
    RadarCore.range_ct -> VirtualArray -> BearingEstimator(n_rx 8, n_doppler 64) at the target's cell, all
    on device buffers: the bearing is bearings_ref's on mimo_ref's output within the estimator's own
    tolerances and nu within 1e-3 of the truth (the raw array is 1e-2 off: tests/test_mimo_host.py); through
    BeamFormer with beams at 0.2 + j / 8, the steered beam holds the maximum at that cell."""
    cube, r, d = chain_cube()
    nv, nd = CH_TX * CH_RX, CH_NC // CH_TX
    rec = np.zeros(1, DET_DTYPE)
    rec["range"], rec["doppler"] = r, d
    w = steering_weights(nv, (CH_NU + np.arange(nv) / nv + 0.5) % 1.0 - 0.5)
    with RadarCore(N_RANGE=NR, N_DOPPLER=CH_NC, N_RX=CH_RX, cfar="none", max_frames=1) as core, \
            VirtualArray(NR, CH_NC, CH_RX, CH_TX) as va, BearingEstimator(NR, nd, nv) as be, \
            BeamFormer(NR, nd, nv, w) as bf:
        dc = DeviceBuffer(cube.nbytes)
        ds = DeviceBuffer(va.frame_bytes())
        dv = DeviceBuffer(va.frame_bytes())
        try:
            dc.upload(cube)
            core.range_ct(dc, ds, 1)
            va.enqueue(ds, 1, dv)
            spec = ds.download(np.complex64, (1, CH_RX, NR, CH_NC))
            virt = dv.download(np.complex64, (1, nv, NR, nd))
            got, snaps = be.estimate(dv, rec)
            maps = bf.form(dv)
        finally:
            for b in (dc, ds, dv):
                b.free()
    assert np.array_equal(spec, range_ct_spectrum(cube, NR, CH_NC, CH_RX))
    ref = M.mimo_ref(spec, CH_TX)
    M.assert_rows_match(virt, ref, label="chain virtual array")
    used = assert_bearings_match(got, snaps, *bearings_ref(ref, rec), label="chain bearing")
    print(f"\nchain: nu {got['nu'][0]:.5f} (truth {CH_NU}), coherence {got['coherence'][0]:.5f}; bearing bounds used: {used}")
    assert abs(float(got["nu"][0]) - CH_NU) <= 1e-3 and got["coherence"][0] >= 0.999
    cell = maps[0, :, r, d].astype(np.float64)
    print(f"chain: other beams / the steered beam at the target's cell: {cell[1:] / cell[0]}")
    assert cell.argmax() == 0, cell
