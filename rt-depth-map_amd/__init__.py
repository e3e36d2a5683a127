"""rt-depth-map_amd: MI355X-native stereo block matching behind rt-depth-map's BlockMatcher.

Import through importlib (the directory name carries the reference's hyphen):
    pkg = importlib.import_module("rt-depth-map_amd")
The compute path is the HIP library rt-depth-map_amd/lib/librtdm_hip.so (C ABI: include/rtdm.h);
nothing in this package falls back to the CPU.

The modules are the host-side mirror of the reference's plugin interfaces, for tests and bench.py, one per handle of the
C ABI (matcher, wls, xyz, morph, rectify, mjpeg, objects, chain) over binding.py and the shared checks of _marshal.py.
``HIPMatcher`` mirrors ``BlockMatcher`` (include/stereo-matcher/stereo-matcher.h:13-19) with the
constructor shape of ``SWMatcherKonolige`` (include/stereo-matcher/bm-sw.h:28-30):
``compute(left, right) -> disp``, ``setROI1``, ``setROI2``.  ``HIPMorphologicalFilter`` mirrors
``VideoFilterDevice`` (include/filter/filter.h:13-37): ``run``, ``getVideoInBuffer`` ...
The C++ adapter that actually plugs into the reference is rt-depth-map_amd/host/bm-hip.{h,cpp}; both
are thin shells over the same C ABI (include/rtdm.h).
"""
from . import binding, synth  # noqa: F401
from .chain import (MEASURE_DTYPE, HIPEstimator, MeasureParams, depth_objects_device, depth_objects_labels_device,  # noqa: F401
                    depth_objects_workspace_bytes, depth_stats_device, distance_cm, estimate_frame, estimate_frame_classes,
                    objects_measure_device, objects_measure_workspace_bytes)
from .matcher import PREFILTER_NORMALIZED_RESPONSE, PREFILTER_XSOBEL, HIPMatcher, HIPSemiGlobalMatcher, create_right_matcher  # noqa: F401
from .mjpeg import HIPMJPEGDecoder, mjpeg_probe  # noqa: F401
from .morph import (MORPH_BLACKHAT, MORPH_CLOSE, MORPH_CROSS, MORPH_DILATE, MORPH_ELLIPSE, MORPH_ERODE, MORPH_GRADIENT,  # noqa: F401
                    MORPH_OPEN, MORPH_OPEN_CLOSE, MORPH_RECT, MORPH_TOPHAT, HIPMorphologicalFilter, get_structuring_element)
from .objects import OBJECT_DTYPE, STATS_DTYPE, HIPObjectDetector, centroids  # noqa: F401
from .rectify import HIPRectifier, init_undistort_rectify_map, load_calibration, stereo_rectify  # noqa: F401
from .synth import synth_pairs_device  # noqa: F401
from .wls import HIPDisparityWLSFilter, create_disparity_wls_filter, wls_params_for  # noqa: F401
from .xyz import POINT_DTYPE, XYZ_FIXED16, XYZ_ROUNDED, HIPReprojector  # noqa: F401
