"""What the seven objects beside fmcw_handle share on the host side (csrc/host_util.hip): how *_create
opens the device and what *_set_grid_for_test says to a null handle.  One parametrised test, so that the
shared paths are pinned once; the per-object test_*_host.py files keep their own checks."""
import ctypes as C

import numpy as np
import pytest

from fmcw import _lib as L

# (symbol stem, configuration type, extra create arguments: the host matrix of n_beams x n_rx = 1 x 1,
#  what the object calls itself in the null-handle message of *_set_grid_for_test)
ONE = np.array([1.0, 0.0], np.float32)
OBJECTS = [
    ("fmcw_plots", "FmcwPlotsConfig", False, b"null plotter"),
    ("fmcw_bearings", "FmcwBearingsConfig", False, b"null bearing estimator"),
    ("fmcw_beams", "FmcwBeamsConfig", True, b"null beamformer"),
    ("fmcw_cacfar", "FmcwCaCfarConfig", False, b"null detector"),
    ("fmcw_tws_dev", "FmcwTwsDevConfig", False, b"null tracker"),
    ("fmcw_cmap", "FmcwCmapConfig", False, b"null clutter map"),
    ("fmcw_adapt", "FmcwAdaptConfig", True, b"null adaptive-weights object"),
]


@pytest.mark.parametrize("sym,cfg_type,matrix,null_text", OBJECTS, ids=[o[0] for o in OBJECTS])
def test_create_opens_the_device_and_null_handle_grid(lib_built, sym, cfg_type, matrix, null_text):
    """The default configuration is valid: without a device *_create is FMCW_ENODEV "no HIP device" and
    leaves the handle null; with one it succeeds, and device_id 63 (no machine has 64 devices) is
    FMCW_ENODEV "out of range".  *_set_grid_for_test(NULL) is FMCW_EINVAL with the object's own text."""
    lib = lib_built
    cfg = getattr(L, cfg_type)()
    getattr(lib, sym + "_config_default")(C.byref(cfg))
    create, destroy = getattr(lib, sym + "_create"), getattr(lib, sym + "_destroy")
    extra = (ONE.ctypes.data,) if matrix else ()
    h = C.c_void_p(1)
    rc = create(C.byref(cfg), *extra, C.byref(h))
    if L.device_count() > 0:
        assert rc == L.FMCW_OK and h.value
        assert destroy(h) == L.FMCW_OK
        cfg.device_id = 63
        h = C.c_void_p(1)
        assert create(C.byref(cfg), *extra, C.byref(h)) == L.FMCW_ENODEV and not h.value
        assert lib.fmcw_last_error() == b"device_id 63 out of range"
    else:
        assert rc == L.FMCW_ENODEV and not h.value
        assert lib.fmcw_last_error() == b"no HIP device"
    assert getattr(lib, sym + "_set_grid_for_test")(None, 1) == L.FMCW_EINVAL
    assert lib.fmcw_last_error() == null_text
