"""ctypes binding of libfmcw.so (include/fmcw.h).

This is the binding a maintainer of the reference's Python tooling (model/) would add:
plain ctypes over the C-ABI, no compiled Python extension.  The library is built in-tree
(``make -C fpga-fmcw-radar-processor_amd``) and loaded from ``lib/libfmcw.so`` next to this
package; it never falls back to anything else -- a missing library is an error.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

PKG_ROOT = Path(__file__).resolve().parent.parent          # fpga-fmcw-radar-processor_amd/
LIB_PATH = Path(os.environ.get("FMCW_LIB", PKG_ROOT / "lib" / "libfmcw.so"))
HEADER_PATH = PKG_ROOT.parent / "include" / "fmcw.h"

# enums (fmcw.h)
FMCW_OK, FMCW_EINVAL, FMCW_ENOMEM, FMCW_EHIP, FMCW_EDETCAP, FMCW_ENODEV = 0, -1, -2, -3, -4, -5
IN_F32, IN_F16, IN_I16 = 0, 1, 2
WIN_NONE, WIN_HAMMING, WIN_Q15_RTL = 0, 1, 2
MAG_ABS, MAG_AMBM = 0, 1
MAP_LINEAR, MAP_DB = 1, 2
CFAR_NONE, CFAR_OS1D, CFAR_OS2D = 0, 1, 2
MTI_OFF, MTI_2PULSE, MTI_3PULSE = 0, 2, 3
COMPAT_CFAR, COMPAT_MTI = 1, 2
SPEC_F32, SPEC_F16, SPEC_S48 = 0, 1, 2
COMM_ID_BYTES = 128
K_RANGE, K_DOPPLER, K_CFAR2D, K_COMPACT, K_COUNT = 0, 1, 2, 3, 4
KERNEL_NAMES = ("k_range", "k_doppler", "k_cfar", "k_compact")
INFO_CHUNK, INFO_RANGE_KERNEL, INFO_WINDOW_SATURATIONS, INFO_WORD_SATURATIONS = 4, 6, 7, 8
INFO_CFAR2D_STEPS = 9
INFO_GRID_RANGE, INFO_GRID_DOPPLER, INFO_GRID_CFAR2D, INFO_GRID_K3B, INFO_GRID_K3C = 10, 11, 12, 13, 14
PARAM_CFAR2D_STEPS = 1   # fmcw_set_param keys
PARAM_GRID_RANGE, PARAM_GRID_DOPPLER, PARAM_GRID_CFAR2D, PARAM_GRID_K3B, PARAM_GRID_K3C = 2, 3, 4, 5, 6
# the persistent grids: the name RadarCore.set_param / .info take -> (FMCW_PARAM_GRID_*, FMCW_INFO_GRID_*)
GRID_KEYS = {"grid_range": (PARAM_GRID_RANGE, INFO_GRID_RANGE), "grid_doppler": (PARAM_GRID_DOPPLER, INFO_GRID_DOPPLER),
             "grid_cfar2d": (PARAM_GRID_CFAR2D, INFO_GRID_CFAR2D), "grid_k3b": (PARAM_GRID_K3B, INFO_GRID_K3B),
             "grid_k3c": (PARAM_GRID_K3C, INFO_GRID_K3C)}
# FMCW_INFO_RANGE_KERNEL 0..3 (1 = round 2's k_range2, retired in ABI 6)
RANGE_KERNELS = ("k_range", "k_range2 (retired)", "k_range_sq", "k_range_px")
STATUS_WORDS = 4      # FMCW_STATUS_WORDS: n_dets_dev = found, lost, window / word saturations
PLOT_STATUS_WORDS = 2  # FMCW_PLOT_STATUS_WORDS: n_plots_dev = plots found, records not examined
BEARING_STATUS_WORDS = 2  # FMCW_BEARING_STATUS_WORDS: n_out_dev = records processed, out of range
CACFAR_CA, CACFAR_GO, CACFAR_SO = 0, 1, 2   # fmcw_cacfar_mode
TWS_DEV_STATUS_WORDS = 2  # FMCW_TWS_DEV_STATUS_WORDS: status_dev = records not examined, out of range
MERGE_STATUS_WORDS = 3   # FMCW_MERGE_STATUS_WORDS: status_dev = merged plots found, records not examined, out of range
UNFOLD_STATUS_WORDS = 4  # FMCW_UNFOLD_STATUS_WORDS: status_dev = reports found, records not examined, out of range, tied
EXCISE_ZERO, EXCISE_INTERP = 0, 1   # fmcw_excise_mode
EXCISE_STATUS_WORDS = 4  # FMCW_EXCISE_STATUS_WORDS: status_dev = samples repaired, lines repaired, samples flagged, lines over half
MIMO_ALIGN_NONE, MIMO_ALIGN_DFT = 0, 1   # fmcw_mimo_align
BEARING_NO_ANGLE, BEARING_ONE_RX, BEARING_OUT_OF_RANGE = 1, 2, 4   # fmcw_bearing.flags bits
DOA_NO_SNAPSHOT, DOA_ONE_CH = 1, 2   # fmcw_doa.flags bits
DOA_MAX_SRC = 4           # FMCW_DOA_MAX_SRC: sources per fmcw_doa record
DOA_STATUS_WORDS = 2      # FMCW_DOA_STATUS_WORDS: n_out_dev = records processed, without a snapshot

STATUS_NAMES = {0: "FMCW_OK", -1: "FMCW_EINVAL", -2: "FMCW_ENOMEM", -3: "FMCW_EHIP",
                -4: "FMCW_EDETCAP", -5: "FMCW_ENODEV"}


class FmcwConfig(C.Structure):
    _fields_ = [
        ("n_range", C.c_uint32), ("n_doppler", C.c_uint32), ("n_rx", C.c_uint32),
        ("in_dtype", C.c_int32), ("window", C.c_int32), ("mag_mode", C.c_int32),
        ("map_kind", C.c_int32), ("cfar_kind", C.c_int32), ("mti_mode", C.c_int32),
        ("cfar1d_ref", C.c_uint32), ("cfar1d_guard", C.c_uint32), ("cfar1d_rank", C.c_uint32),
        ("cfar1d_alpha", C.c_float),
        ("cfar2d_ref_range", C.c_uint32), ("cfar2d_guard_range", C.c_uint32),
        ("cfar2d_ref_doppler", C.c_uint32), ("cfar2d_guard_doppler", C.c_uint32),
        ("cfar2d_rank_pct", C.c_uint32), ("cfar2d_scale_min", C.c_uint32),
        ("cfar2d_scale_nom", C.c_uint32), ("cfar2d_scale_max", C.c_uint32),
        ("cfar2d_scale_override", C.c_uint32),
        ("max_frames", C.c_uint32), ("chunk_frames", C.c_uint32), ("device_id", C.c_int32),
        ("compat_rtl", C.c_uint32), ("range_shift", C.c_uint32), ("spectrum_dtype", C.c_int32),
        ("det_capacity", C.c_uint32),
    ]


class FmcwDet(C.Structure):
    _fields_ = [("frame", C.c_uint32), ("range", C.c_uint16), ("doppler", C.c_uint16),
                ("mag", C.c_float), ("threshold", C.c_float)]


class FmcwPlot(C.Structure):
    _fields_ = [("frame", C.c_uint32), ("range", C.c_uint16), ("doppler", C.c_uint16),
                ("mag", C.c_float), ("threshold", C.c_float), ("n_cells", C.c_uint32),
                ("sum_mag", C.c_float), ("d_range", C.c_float), ("d_doppler", C.c_float)]


class FmcwPlotsConfig(C.Structure):
    _fields_ = [("n_range", C.c_uint32), ("n_doppler", C.c_uint32), ("win_range", C.c_uint32),
                ("win_doppler", C.c_uint32), ("max_dets", C.c_uint32), ("device_id", C.c_int32)]


class FmcwMplot(C.Structure):
    _fields_ = [("frame", C.c_uint32), ("range", C.c_uint16), ("doppler", C.c_uint16),
                ("mag", C.c_float), ("beam", C.c_uint16), ("n_merged", C.c_uint16),
                ("sum_mag", C.c_float), ("d_beam", C.c_float), ("d_range", C.c_float),
                ("d_doppler", C.c_float)]


class FmcwMergeConfig(C.Structure):
    _fields_ = [("n_range", C.c_uint32), ("n_doppler", C.c_uint32), ("n_beams", C.c_uint32),
                ("win_beam", C.c_uint32), ("win_range", C.c_uint32), ("win_doppler", C.c_uint32),
                ("beam_wrap", C.c_uint32), ("max_recs", C.c_uint32), ("max_maps", C.c_uint32),
                ("device_id", C.c_int32)]


class FmcwVplot(C.Structure):
    _fields_ = [("frame", C.c_uint32), ("range", C.c_uint16), ("doppler", C.c_uint16),
                ("mag", C.c_float), ("v_fine", C.c_int32), ("fold", C.c_int16), ("n_hits", C.c_uint8),
                ("hit_mask", C.c_uint8), ("sum_mag", C.c_float), ("pos", C.c_uint16),
                ("n_ties", C.c_uint16), ("src", C.c_uint32)]


class FmcwUnfoldConfig(C.Structure):
    _fields_ = [("n_range", C.c_uint32), ("n_doppler", C.c_uint32), ("n_prf", C.c_uint32),
                ("prf_units", C.c_uint32 * 8), ("prf_phase", C.c_uint32), ("step", C.c_uint32),
                ("zero_bin", C.c_uint32), ("v_max", C.c_uint32), ("out_unit", C.c_uint32),
                ("tol_range", C.c_uint32), ("tol_doppler", C.c_uint32), ("m_of", C.c_uint32),
                ("n_streams", C.c_uint32), ("max_recs", C.c_uint32), ("max_frames", C.c_uint32),
                ("device_id", C.c_int32)]


class FmcwBearing(C.Structure):
    _fields_ = [("frame", C.c_uint32), ("range", C.c_uint16), ("doppler", C.c_uint16),
                ("flags", C.c_uint32), ("nu", C.c_float), ("sin_theta", C.c_float),
                ("power", C.c_float), ("coherence", C.c_float), ("reserved", C.c_uint32)]


class FmcwBearingsConfig(C.Structure):
    _fields_ = [("n_range", C.c_uint32), ("n_doppler", C.c_uint32), ("n_rx", C.c_uint32),
                ("window", C.c_int32), ("mti_mode", C.c_int32), ("spacing", C.c_float),
                ("max_records", C.c_uint32), ("device_id", C.c_int32)]


class FmcwBeamsConfig(C.Structure):
    _fields_ = [("n_range", C.c_uint32), ("n_doppler", C.c_uint32), ("n_rx", C.c_uint32),
                ("n_beams", C.c_uint32), ("window", C.c_int32), ("mti_mode", C.c_int32),
                ("reserved", C.c_uint32), ("device_id", C.c_int32)]


class FmcwAdaptConfig(C.Structure):
    _fields_ = [("n_range", C.c_uint32), ("n_doppler", C.c_uint32), ("n_rx", C.c_uint32),
                ("n_beams", C.c_uint32), ("mti_mode", C.c_int32), ("train_r0", C.c_uint32),
                ("train_rows", C.c_uint32), ("loading", C.c_float), ("reserved", C.c_uint32),
                ("device_id", C.c_int32)]


class FmcwCaCfarConfig(C.Structure):
    _fields_ = [("n_range", C.c_uint32), ("n_doppler", C.c_uint32), ("mode", C.c_int32),
                ("ref_range", C.c_uint32), ("guard_range", C.c_uint32), ("ref_doppler", C.c_uint32),
                ("guard_doppler", C.c_uint32), ("alpha", C.c_float), ("max_frames", C.c_uint32),
                ("device_id", C.c_int32), ("reserved", C.c_uint32 * 2)]


class FmcwExciseConfig(C.Structure):
    _fields_ = [("n_range", C.c_uint32), ("n_doppler", C.c_uint32), ("n_rx", C.c_uint32),
                ("in_dtype", C.c_int32), ("mode", C.c_int32), ("guard", C.c_uint32),
                ("rank_pct", C.c_uint32), ("alpha", C.c_float), ("max_frames", C.c_uint32),
                ("device_id", C.c_int32), ("reserved", C.c_uint32 * 2)]


class FmcwMimoConfig(C.Structure):
    _fields_ = [("n_range", C.c_uint32), ("n_chirps", C.c_uint32), ("n_rx", C.c_uint32),
                ("n_tx", C.c_uint32), ("align", C.c_int32), ("reserved", C.c_uint32 * 2),
                ("device_id", C.c_int32)]


class FmcwDoaSrc(C.Structure):
    _fields_ = [("grid", C.c_uint32), ("pos", C.c_float), ("amp_re", C.c_float), ("amp_im", C.c_float)]


class FmcwDoa(C.Structure):
    _fields_ = [("frame", C.c_uint32), ("range", C.c_uint16), ("doppler", C.c_uint16),
                ("flags", C.c_uint32), ("n_src", C.c_uint32), ("total", C.c_float),
                ("residual", C.c_float), ("reserved", C.c_uint32 * 2), ("src", FmcwDoaSrc * 4)]


class FmcwDoaConfig(C.Structure):
    _fields_ = [("n_ch", C.c_uint32), ("n_grid", C.c_uint32), ("k_max", C.c_uint32),
                ("relax_passes", C.c_uint32), ("min_rel", C.c_float), ("refine", C.c_uint32),
                ("max_records", C.c_uint32), ("device_id", C.c_int32)]


class FmcwCmapConfig(C.Structure):
    _fields_ = [("n_range", C.c_uint32), ("n_doppler", C.c_uint32), ("n_streams", C.c_uint32),
                ("gain", C.c_float), ("alpha", C.c_float), ("floor", C.c_float), ("clip", C.c_float),
                ("spread_range", C.c_uint32), ("spread_doppler", C.c_uint32), ("warmup", C.c_uint32),
                ("max_frames", C.c_uint32), ("device_id", C.c_int32), ("reserved", C.c_uint32 * 4)]


class FmcwTwsConfig(C.Structure):
    _fields_ = [("max_tracks", C.c_uint32), ("max_dets", C.c_uint32), ("init_hits", C.c_uint32),
                ("coast_max", C.c_uint32), ("gate_r", C.c_uint32), ("gate_d", C.c_uint32),
                ("alpha_q8", C.c_uint32), ("beta_q8", C.c_uint32), ("rtl_compat", C.c_int32)]


class FmcwTwsDevConfig(C.Structure):
    _fields_ = [("tws", FmcwTwsConfig), ("n_streams", C.c_uint32), ("max_scans", C.c_uint32),
                ("device_id", C.c_int32)]


class FmcwTrack(C.Structure):
    _fields_ = [("id", C.c_uint16), ("status", C.c_uint8), ("quality", C.c_uint8),
                ("range_q2", C.c_int32), ("doppler_q2", C.c_int32), ("vel_r", C.c_int32),
                ("vel_d", C.c_int32), ("last_mag", C.c_uint32), ("age", C.c_uint32)]


# every symbol include/fmcw.h declares, with its ctypes signature
_VP, _SZ, _I, _U32P = C.c_void_p, C.c_size_t, C.c_int, C.POINTER(C.c_uint32)
SIGNATURES = {
    "fmcw_version": (C.c_char_p, []),
    "fmcw_abi_version": (_I, []),
    "fmcw_last_error": (C.c_char_p, []),
    "fmcw_config_default": (None, [C.POINTER(FmcwConfig)]),
    "fmcw_create": (_I, [C.POINTER(FmcwConfig), C.POINTER(_VP)]),
    "fmcw_destroy": (_I, [_VP]),
    "fmcw_enqueue": (_I, [_VP, _VP, _SZ, _VP, _VP, _SZ, _VP, _VP]),
    "fmcw_process": (_I, [_VP, _VP, _SZ, _VP, _VP, _SZ, C.POINTER(_SZ), _VP]),
    "fmcw_range_ct": (_I, [_VP, _VP, _SZ, _VP, _VP]),
    "fmcw_magnitude": (_I, [_VP, _VP, _SZ, _I, _VP]),
    "fmcw_cfar": (_I, [_VP, _VP, _SZ, _VP, _SZ, _VP, _VP]),
    "fmcw_set_profiling": (_I, [_VP, _I]),
    "fmcw_get_info": (_I, [_VP, _I, C.POINTER(C.c_int64)]),
    "fmcw_set_param": (_I, [_VP, _I, C.c_int64]),
    "fmcw_kernel_times": (_I, [_VP, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]),
    "fmcw_reset_kernel_times": (_I, [_VP]),
    "fmcw_device_alloc": (_I, [_SZ, C.POINTER(_VP), _I]),
    "fmcw_device_free": (_I, [_VP]),
    "fmcw_memcpy": (_I, [_VP, _VP, _SZ, _I]),
    "fmcw_device_count": (_I, [C.POINTER(_I)]),
    "fmcw_comm_unique_id": (_I, [_VP]),
    "fmcw_comm_create": (_I, [_VP, _I, _I, _I, _SZ, C.POINTER(_VP)]),
    "fmcw_comm_destroy": (_I, [_VP]),
    "fmcw_comm_info": (_I, [_VP, C.POINTER(_I), C.POINTER(_I), C.POINTER(_I), C.POINTER(_SZ)]),
    "fmcw_gather_dets": (_I, [_VP, _VP, _SZ, _VP, C.c_uint32, _VP, _VP, _I, _VP]),
    "fmcw_comm_fail_next_alloc_for_test": (_I, [_I]),
    "fmcw_comm_check_decide_for_test": (_I, [C.POINTER(C.c_uint64), _I, _SZ]),
    "fmcw_gather_pack_for_test": (_I, [_VP, _SZ, _VP, _SZ, C.c_uint32, _VP, _VP]),
    "fmcw_gather_compact_for_test": (_I, [_VP, _I, _SZ, _VP, _VP, _VP]),
    "fmcw_plots_config_default": (None, [C.POINTER(FmcwPlotsConfig)]),
    "fmcw_plots_create": (_I, [C.POINTER(FmcwPlotsConfig), C.POINTER(_VP)]),
    "fmcw_plots_destroy": (_I, [_VP]),
    "fmcw_plots_enqueue": (_I, [_VP, _VP, _SZ, _VP, _VP, _SZ, _VP, _VP]),
    "fmcw_plots_set_grid_for_test": (_I, [_VP, C.c_uint32]),
    "fmcw_merge_config_default": (None, [C.POINTER(FmcwMergeConfig)]),
    "fmcw_merge_create": (_I, [C.POINTER(FmcwMergeConfig), C.POINTER(_VP)]),
    "fmcw_merge_destroy": (_I, [_VP]),
    "fmcw_merge_enqueue": (_I, [_VP, _VP, _SZ, _SZ, _VP, _SZ, _VP, _SZ, _VP, _VP]),
    "fmcw_merge_set_grid_for_test": (_I, [_VP, C.c_uint32]),
    "fmcw_unfold_config_default": (None, [C.POINTER(FmcwUnfoldConfig)]),
    "fmcw_unfold_create": (_I, [C.POINTER(FmcwUnfoldConfig), C.POINTER(_VP)]),
    "fmcw_unfold_destroy": (_I, [_VP]),
    "fmcw_unfold_enqueue": (_I, [_VP, _VP, _SZ, _SZ, _VP, _SZ, _VP, _SZ, _VP, _VP]),
    "fmcw_unfold_set_grid_for_test": (_I, [_VP, C.c_uint32]),
    "fmcw_bearings_config_default": (None, [C.POINTER(FmcwBearingsConfig)]),
    "fmcw_bearings_create": (_I, [C.POINTER(FmcwBearingsConfig), C.POINTER(_VP)]),
    "fmcw_bearings_destroy": (_I, [_VP]),
    "fmcw_bearings_enqueue": (_I, [_VP, _VP, _SZ, _VP, _SZ, _SZ, _VP, _VP, _VP, _VP, _VP]),
    "fmcw_bearings_set_grid_for_test": (_I, [_VP, C.c_uint32]),
    "fmcw_beams_config_default": (None, [C.POINTER(FmcwBeamsConfig)]),
    "fmcw_beams_create": (_I, [C.POINTER(FmcwBeamsConfig), _VP, C.POINTER(_VP)]),
    "fmcw_beams_destroy": (_I, [_VP]),
    "fmcw_beams_enqueue": (_I, [_VP, _VP, _SZ, _VP, _VP]),
    "fmcw_beams_set_grid_for_test": (_I, [_VP, C.c_uint32]),
    "fmcw_beams_set_weights_dev": (_I, [_VP, _VP, _VP]),
    "fmcw_adapt_config_default": (None, [C.POINTER(FmcwAdaptConfig)]),
    "fmcw_adapt_create": (_I, [C.POINTER(FmcwAdaptConfig), _VP, C.POINTER(_VP)]),
    "fmcw_adapt_destroy": (_I, [_VP]),
    "fmcw_adapt_enqueue": (_I, [_VP, _VP, _SZ, _VP, _VP, _VP, _VP]),
    "fmcw_adapt_set_grid_for_test": (_I, [_VP, C.c_uint32]),
    "fmcw_cacfar_config_default": (None, [C.POINTER(FmcwCaCfarConfig)]),
    "fmcw_cacfar_create": (_I, [C.POINTER(FmcwCaCfarConfig), C.POINTER(_VP)]),
    "fmcw_cacfar_destroy": (_I, [_VP]),
    "fmcw_cacfar_enqueue": (_I, [_VP, _VP, _SZ, _VP, _SZ, _VP, _VP]),
    "fmcw_cacfar_set_grid_for_test": (_I, [_VP, C.c_uint32]),
    "fmcw_excise_config_default": (None, [C.POINTER(FmcwExciseConfig)]),
    "fmcw_excise_create": (_I, [C.POINTER(FmcwExciseConfig), C.POINTER(_VP)]),
    "fmcw_excise_destroy": (_I, [_VP]),
    "fmcw_excise_enqueue": (_I, [_VP, _VP, _SZ, _VP, _VP, _VP, _VP, _VP]),
    "fmcw_excise_set_grid_for_test": (_I, [_VP, C.c_uint32]),
    "fmcw_mimo_config_default": (None, [C.POINTER(FmcwMimoConfig)]),
    "fmcw_mimo_create": (_I, [C.POINTER(FmcwMimoConfig), C.POINTER(_VP)]),
    "fmcw_mimo_destroy": (_I, [_VP]),
    "fmcw_mimo_enqueue": (_I, [_VP, _VP, _SZ, _VP, _VP]),
    "fmcw_mimo_set_grid_for_test": (_I, [_VP, C.c_uint32]),
    "fmcw_doa_config_default": (None, [C.POINTER(FmcwDoaConfig)]),
    "fmcw_doa_create": (_I, [C.POINTER(FmcwDoaConfig), C.POINTER(_VP)]),
    "fmcw_doa_destroy": (_I, [_VP]),
    "fmcw_doa_set_steering": (_I, [_VP, _VP, _VP]),
    "fmcw_doa_set_steering_dev": (_I, [_VP, _VP, _VP]),
    "fmcw_doa_enqueue": (_I, [_VP, _VP, _VP, _SZ, _SZ, _VP, _VP, _VP, _VP, _VP]),
    "fmcw_doa_set_grid_for_test": (_I, [_VP, C.c_uint32]),
    "fmcw_cmap_config_default": (None, [C.POINTER(FmcwCmapConfig)]),
    "fmcw_cmap_create": (_I, [C.POINTER(FmcwCmapConfig), C.POINTER(_VP)]),
    "fmcw_cmap_destroy": (_I, [_VP]),
    "fmcw_cmap_enqueue": (_I, [_VP, _VP, _SZ, _VP, _SZ, _VP, _VP]),
    "fmcw_cmap_reset": (_I, [_VP, _VP]),
    "fmcw_cmap_get_state": (_I, [_VP, _VP, _VP, _VP]),
    "fmcw_cmap_set_state": (_I, [_VP, _VP, _VP, _VP]),
    "fmcw_cmap_set_grid_for_test": (_I, [_VP, C.c_uint32]),
    "fmcw_tws_config_default": (None, [C.POINTER(FmcwTwsConfig)]),
    "fmcw_tws_create": (_I, [C.POINTER(FmcwTwsConfig), C.POINTER(_VP)]),
    "fmcw_tws_destroy": (_I, [_VP]),
    "fmcw_tws_scan": (_I, [_VP, _VP, _SZ, C.POINTER(FmcwTrack), _SZ, C.POINTER(_SZ), _U32P]),
    "fmcw_tws_dev_config_default": (None, [C.POINTER(FmcwTwsDevConfig)]),
    "fmcw_tws_dev_create": (_I, [C.POINTER(FmcwTwsDevConfig), C.POINTER(_VP)]),
    "fmcw_tws_dev_destroy": (_I, [_VP]),
    "fmcw_tws_dev_reset": (_I, [_VP, _VP]),
    "fmcw_tws_dev_enqueue": (_I, [_VP, _VP, _SZ, _SZ, _VP, _SZ, _VP, _SZ, _VP, _VP, _VP]),
    "fmcw_tws_dev_set_grid_for_test": (_I, [_VP, C.c_uint32]),
}

_lib = None


class FmcwError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"{STATUS_NAMES.get(code, code)}: {msg}")
        self.code = code


def load() -> C.CDLL:
    """Load libfmcw.so (once).  Raises if it has not been built -- no fallback exists."""
    global _lib
    if _lib is None:
        if not LIB_PATH.exists():
            raise FileNotFoundError(
                f"{LIB_PATH} not built: run `make -C {PKG_ROOT}` or __graft_entry__.build()")
        lib = C.CDLL(str(LIB_PATH))
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


def check(code: int) -> int:
    if code != FMCW_OK:
        raise FmcwError(code, load().fmcw_last_error().decode(errors="replace"))
    return code


def default_config() -> FmcwConfig:
    cfg = FmcwConfig()
    load().fmcw_config_default(C.byref(cfg))
    return cfg


def device_count() -> int:
    n = C.c_int(0)
    load().fmcw_device_count(C.byref(n))
    return n.value
