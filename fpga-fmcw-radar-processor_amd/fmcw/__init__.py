"""fmcw -- MI355X-native FMCW range-Doppler + OS-CFAR hot path (host side).

The compute runs in libfmcw.so (hand-written HIP for gfx950, include/fmcw.h); this package
is the thin host shim the reference's Python tooling (model/) would call, mirroring the
reference's radar_core interface (rtl/src/radar_core.vhd:11-57).
"""
from ._lib import FmcwError, load, device_count, LIB_PATH, HEADER_PATH  # noqa: F401
from .radar_core import RadarCore, RadarOutput, DeviceBuffer, DET_DTYPE, magnitude  # noqa: F401
from .radar_core import pack_adc_words, adc_words_to_cube  # noqa: F401
from .tracker import TwsTracker, TRACK_DTYPE  # noqa: F401
from .tracker_dev import DeviceTwsTracker  # noqa: F401
from .plots import PlotExtractor, PLOT_DTYPE  # noqa: F401
from .merge import BeamMerger, MPLOT_DTYPE  # noqa: F401
from .unfold import VelocityUnfolder, VPLOT_DTYPE, velocity_mps  # noqa: F401
from .bearings import BearingEstimator, BEARING_DTYPE  # noqa: F401
from .beams import BeamFormer, steering_weights  # noqa: F401
from .adapt import AdaptiveWeights, steering_vectors, ADAPT_FALLBACK  # noqa: F401
from .cacfar import CaCfar  # noqa: F401
from .cmap import ClutterMap  # noqa: F401
from .excise import InterferenceExciser  # noqa: F401
from .mimo import VirtualArray  # noqa: F401
from .doa import AngleResolver, DOA_DTYPE, line_steering, planar_steering, calibrated  # noqa: F401
from . import synth, formats  # noqa: F401

__all__ = ["AngleResolver", "DOA_DTYPE", "line_steering", "planar_steering", "calibrated", "VirtualArray", "InterferenceExciser", "VelocityUnfolder", "VPLOT_DTYPE", "velocity_mps", "BeamMerger", "MPLOT_DTYPE", "AdaptiveWeights", "steering_vectors", "ADAPT_FALLBACK", "ClutterMap", "DeviceTwsTracker", "CaCfar", "BeamFormer", "steering_weights", "BearingEstimator", "BEARING_DTYPE", "PlotExtractor", "PLOT_DTYPE", "RadarCore", "RadarOutput", "DeviceBuffer", "DET_DTYPE", "FmcwError", "load",
           "device_count", "magnitude", "TwsTracker", "TRACK_DTYPE", "synth", "formats", "pack_adc_words", "adc_words_to_cube"]
