"""rt-depth-map_amd: MI355X-native stereo block matching behind rt-depth-map's BlockMatcher.

Import through importlib (the directory name carries the reference's hyphen):
    pkg = importlib.import_module("rt-depth-map_amd")
The compute path is the HIP library rt-depth-map_amd/lib/librtdm_hip.so (C ABI: include/rtdm.h);
nothing in this package falls back to the CPU.
"""
from . import binding, synth  # noqa: F401
from .matcher import (MORPH_BLACKHAT, MORPH_CLOSE, MORPH_CROSS, MORPH_DILATE, MORPH_ELLIPSE, MORPH_ERODE, MORPH_GRADIENT,  # noqa: F401
                      MORPH_OPEN, MORPH_OPEN_CLOSE, MORPH_RECT, MORPH_TOPHAT, OBJECT_DTYPE, POINT_DTYPE, PREFILTER_NORMALIZED_RESPONSE, PREFILTER_XSOBEL, XYZ_FIXED16, XYZ_ROUNDED,  # noqa: F401
                      HIPDisparityWLSFilter, HIPEstimator, HIPMatcher, HIPMJPEGDecoder, HIPMorphologicalFilter, HIPObjectDetector,  # noqa: F401
                      HIPReprojector, HIPRectifier, HIPSemiGlobalMatcher, create_disparity_wls_filter, create_right_matcher,
                      depth_objects_device, depth_objects_workspace_bytes, depth_stats_device, estimate_frame, estimate_frame_classes, get_structuring_element, init_undistort_rectify_map, load_calibration, mjpeg_probe, stereo_rectify,
                      synth_pairs_device, wls_params_for)
