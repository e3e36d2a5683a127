"""ctypes binding of the C ABI in include/rtdm.h (librtdm_hip.so).

This is plumbing for tests and bench.py: it passes raw pointers (numpy buffers or
torch ``data_ptr()``) straight to the C entry points.  There is no Python or CPU fallback: if the
library is missing, or no HIP device is usable, loading / creating fails loudly.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "librtdm_hip.so")

RTDM_OK = 0
STATUS = {0: "RTDM_OK", -1: "RTDM_ERR_BAD_PARAM", -2: "RTDM_ERR_BAD_SIZE", -3: "RTDM_ERR_NO_DEVICE",
          -4: "RTDM_ERR_HIP", -5: "RTDM_ERR_NOMEM", -6: "RTDM_ERR_UNSUPPORTED", -7: "RTDM_ERR_NULL", -8: "RTDM_ERR_BAD_STREAM"}
STAGES = ("prefilter", "search", "lrcheck", "speckle")
PREFILTER_NORMALIZED_RESPONSE, PREFILTER_XSOBEL = 0, 1   # cv::StereoBM's values (RTDM_PREFILTER_* in rtdm.h)
SGM_COST_BT, SGM_COST_CENSUS = 0, 1                      # RTDM_SGM_COST_* in rtdm.h


class RtdmError(RuntimeError):
    def __init__(self, status, where, detail=""):
        self.status = status
        super().__init__("%s failed: %s (%d) %s" % (where, STATUS.get(status, "?"), status, detail))


class Region(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("x", "y", "width", "height")]


class HsvRange(C.Structure):
    _fields_ = [("low", C.c_int * 3), ("high", C.c_int * 3)]


class Object(C.Structure):              # rtdm_object, 32 bytes
    _fields_ = [(n, C.c_int) for n in ("x", "y", "width", "height", "cls", "first_pixel")] + [("reserved", C.c_int * 2)]


class ObjectStats(C.Structure):         # rtdm_object_stats, 48 bytes
    _fields_ = [(n, C.c_int64) for n in ("m00", "m10", "m01", "m20", "m11", "m02")]


class MeasureParams(C.Structure):       # rtdm_measure_params
    _fields_ = [("disparity_mode", C.c_int), ("max_z", C.c_double), ("nquant", C.c_int), ("permille", C.c_int * 8)]


class ObjectMeasure(C.Structure):       # rtdm_object_measure, 88 bytes
    _fields_ = [("npix", C.c_int32), ("nplane", C.c_int32), ("zq", C.c_float * 8), ("lo", C.c_float * 3), ("hi", C.c_float * 3),
                ("mean", C.c_double * 3)]


MAX_HSV_RANGES, MAX_CLASSES = 16, 8      # RTDM_MAX_HSV_RANGES, RTDM_MAX_CLASSES
MAX_REGIONS = 64                         # RTDM_MAX_REGIONS: objects of a frame that get a depth


class SGMParams(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("blockSize", "minDisparity", "numDisparities", "P1", "P2", "uniquenessRatio",
                                       "speckleWindowSize", "speckleRange", "disp12MaxDiff", "paths")]


class BMParams(C.Structure):
    _fields_ = [(n, C.c_int) for n in (
        "preFilterCap", "blockSize", "minDisparity", "numDisparities", "textureThreshold",
        "uniquenessRatio", "speckleWindowSize", "speckleRange", "disp12MaxDiff", "legacy_right_clamp")]


class WLSParams(C.Structure):
    _fields_ = [("lambda_", C.c_double), ("sigma_color", C.c_double)] + [(n, C.c_int) for n in (
        "lrc_thresh", "depth_discontinuity_radius", "min_disparity", "num_disparities", "roi_left", "roi_right", "roi_top",
        "roi_bottom", "num_iter")] + [("attenuation", C.c_double), ("use_confidence", C.c_int)]


class XYZParams(C.Structure):
    _fields_ = [("Q", C.c_double * 16), ("disparity_mode", C.c_int), ("handle_missing_values", C.c_int),
                ("min_disparity", C.c_int), ("max_z", C.c_double)]


class Point(C.Structure):               # rtdm_point, 16 bytes
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("z", C.c_float)] + [(n, C.c_uint8) for n in "rgba"]


XYZ_FIXED16, XYZ_ROUNDED = 0, 1          # RTDM_XYZ_* in rtdm.h


class MJPEGInfo(C.Structure):           # rtdm_mjpeg_info
    _fields_ = [(n, C.c_int) for n in ("width", "height", "components", "h_samp", "v_samp", "restart_interval", "segments",
                                       "has_dht")]


class Calib(C.Structure):               # rtdm_calib
    _fields_ = [("M1", C.c_double * 9), ("D1", C.c_double * 14), ("M2", C.c_double * 9), ("D2", C.c_double * 14),
                ("R", C.c_double * 9), ("T", C.c_double * 3), ("width", C.c_int), ("height", C.c_int)]


class Rectification(C.Structure):       # rtdm_rectification
    _fields_ = [("R1", C.c_double * 9), ("R2", C.c_double * 9), ("P1", C.c_double * 12), ("P2", C.c_double * 12),
                ("Q", C.c_double * 16), ("roi1", Region), ("roi2", Region)]


CALIB_ZERO_DISPARITY = 1024              # RTDM_CALIB_ZERO_DISPARITY
CALIB_HAS = {"Width": 1, "Height": 2, "ROI1": 4, "ROI2": 8, "R1": 16, "R2": 32, "P1": 64, "P2": 128, "Q": 256}   # RTDM_CALIB_HAS_*

MORPH_RECT, MORPH_CROSS, MORPH_ELLIPSE = 0, 1, 2          # cv::MorphShapes (RTDM_MORPH_* in rtdm.h)
MORPH_ERODE, MORPH_DILATE, MORPH_OPEN, MORPH_CLOSE, MORPH_GRADIENT, MORPH_TOPHAT, MORPH_BLACKHAT = range(7)   # cv::MorphTypes
MORPH_OPEN_CLOSE = 100                                    # SWMorphologicalFilter::run, the default
MORPH_MAX_SIZE = 63


class MorphElement(C.Structure):        # rtdm_morph_element
    _fields_ = [(n, C.c_int) for n in ("width", "height", "anchor_x", "anchor_y")] + [("mask", C.c_uint8 * (MORPH_MAX_SIZE * MORPH_MAX_SIZE))]


vp, u8p, i16p, u16p, sz = C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t
SIGNATURES = {          # every entry point of include/rtdm.h: (restype, argtypes)
    "rtdm_strerror": (C.c_char_p, [C.c_int]),
    "rtdm_last_hip_error": (C.c_char_p, []),
    "rtdm_abi_version": (C.c_int, []),
    "rtdm_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "rtdm_bm_default_params": (None, [C.POINTER(BMParams), C.c_int]),
    "rtdm_bm_create": (C.c_int, [C.POINTER(BMParams), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(vp)]),
    "rtdm_bm_destroy": (None, [vp]),
    "rtdm_bm_set_roi": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "rtdm_bm_get_params": (C.c_int, [vp, C.POINTER(BMParams)]),
    "rtdm_bm_set_prefilter": (C.c_int, [vp, C.c_int, C.c_int]),
    "rtdm_bm_get_prefilter": (C.c_int, [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "rtdm_bm_compute": (C.c_int, [vp, u8p, sz, u8p, sz, C.c_int, C.c_int, i16p, sz]),
    "rtdm_bm_compute_device": (C.c_int, [vp, C.c_int, u8p, u8p, sz, sz, C.c_int, C.c_int, i16p, sz, sz, vp]),
    "rtdm_bm_compute_device_rois": (C.c_int, [vp, C.c_int, u8p, u8p, sz, sz, C.c_int, C.c_int, vp, i16p, sz, sz, vp]),
    "rtdm_bm_compute_batch": (C.c_int, [vp, C.c_int, u8p, u8p, sz, sz, C.c_int, C.c_int, i16p, sz, sz]),
    "rtdm_bm_synchronize": (C.c_int, [vp]),
    "rtdm_bm_set_profiling": (C.c_int, [vp, C.c_int]),
    "rtdm_bm_get_stage_time": (C.c_int, [vp, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_long), C.POINTER(C.c_long)]),
    "rtdm_bm_reset_stage_times": (C.c_int, [vp]),
    "rtdm_bm_search_variant": (C.c_char_p, [vp]),
    "rtdm_bm_get_tuner_stats": (C.c_int, [vp, C.POINTER(C.c_long), C.POINTER(C.c_long)]),
    "rtdm_debug_search_kernel": (None, [C.c_int]),
    "rtdm_debug_disparity_slice": (None, [C.c_int]),
    "rtdm_morph_make_element": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(MorphElement)]),
    "rtdm_morph_set_op": (C.c_int, [vp, C.c_int, C.c_int, C.POINTER(MorphElement)]),
    "rtdm_morph_get_op": (C.c_int, [vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(MorphElement)]),
    "rtdm_objects_set_morph": (C.c_int, [vp, C.c_int, C.c_int, C.POINTER(MorphElement)]),
    "rtdm_objects_get_morph": (C.c_int, [vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(MorphElement)]),
    "rtdm_debug_morph_general": (None, [C.c_int]),
    "rtdm_morph_create": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(vp)]),
    "rtdm_morph_destroy": (None, [vp]),
    "rtdm_morph_in_buffer": (vp, [vp]),
    "rtdm_morph_out_buffer": (vp, [vp]),
    "rtdm_morph_run": (C.c_int, [vp, u8p, sz, u8p, sz, C.c_int, C.c_int]),
    "rtdm_morph_run_device": (C.c_int, [vp, C.c_int, u8p, sz, sz, u8p, sz, sz, C.c_int, C.c_int, vp]),
    "rtdm_sgm_default_params": (None, [C.POINTER(SGMParams), C.c_int, C.c_int]),
    "rtdm_sgm_create": (C.c_int, [C.POINTER(SGMParams), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(vp)]),
    "rtdm_sgm_destroy": (None, [vp]),
    "rtdm_sgm_compute": (C.c_int, [vp, u8p, sz, u8p, sz, C.c_int, C.c_int, i16p, sz]),
    "rtdm_sgm_compute_device": (C.c_int, [vp, C.c_int, u8p, u8p, sz, sz, C.c_int, C.c_int, i16p, sz, sz, vp]),
    "rtdm_sgm_get_pass_stats": (C.c_int, [vp, C.POINTER(C.c_long), C.POINTER(C.c_int)]),
    "rtdm_sgm_path_variant": (C.c_char_p, [vp]),
    "rtdm_debug_sgm_wide_paths": (None, [C.c_int]),
    "rtdm_sgm_set_prefilter_cap": (C.c_int, [vp, C.c_int]),
    "rtdm_sgm_compute_cn": (C.c_int, [vp, C.c_int, u8p, sz, u8p, sz, C.c_int, C.c_int, i16p, sz]),
    "rtdm_sgm_compute_device_cn": (C.c_int, [vp, C.c_int, C.c_int, u8p, u8p, sz, sz, C.c_int, C.c_int, i16p, sz, sz, vp]),
    "rtdm_debug_sgm_cost16": (None, [C.c_int]),
    "rtdm_sgm_set_cost": (C.c_int, [vp, C.c_int, C.c_int, C.c_int]),
    "rtdm_sgm_get_cost": (C.c_int, [vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "rtdm_sgm_set_mode": (C.c_int, [vp, C.c_int]),
    "rtdm_sgm_get_mode": (C.c_int, [vp, C.POINTER(C.c_int)]),
    "rtdm_bm_compute_depth": (C.c_int, [vp, u8p, sz, u8p, sz, C.c_int, C.c_int, C.POINTER(C.c_double), u8p, sz,
                                        C.POINTER(Region), C.c_int, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_int), i16p, sz]),
    "rtdm_depth_stats_device": (C.c_int, [C.c_int, i16p, sz, C.c_int, C.c_int, C.POINTER(C.c_double), u8p, sz,
                                          C.POINTER(Region), C.c_int, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_int), vp]),
    "rtdm_rectify_create": (C.c_int, [i16p, u16p, i16p, u16p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                      C.c_int, C.c_int, C.POINTER(vp)]),
    "rtdm_rectify_destroy": (None, [vp]),
    "rtdm_rectify_gray": (C.c_int, [vp, u8p, sz, u8p, sz, u8p, sz, u8p, sz]),
    "rtdm_rectify_rgb": (C.c_int, [vp, C.c_int, u8p, sz, u8p, sz]),
    "rtdm_rectify_gray_device": (C.c_int, [vp, C.c_int, u8p, u8p, u8p, u8p, vp]),
    "rtdm_bm_compute_rgb": (C.c_int, [vp, vp, u8p, sz, u8p, sz, i16p, sz]),
    "rtdm_bm_compute_rgb_device": (C.c_int, [vp, vp, C.c_int, u8p, u8p, i16p, vp]),
    "rtdm_calib_load": (C.c_int, [C.c_char_p, C.c_char_p, C.POINTER(Calib), C.POINTER(Rectification), C.POINTER(C.c_uint)]),
    "rtdm_stereo_rectify": (C.c_int, [C.POINTER(Calib), C.c_int, C.c_double, C.c_int, C.c_int, C.POINTER(Rectification)]),
    "rtdm_undistort_rectify_map": (C.c_int, [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, i16p, u16p]),
    "rtdm_undistort_rectify_map_device": (C.c_int, [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, i16p, u16p, vp]),
    "rtdm_rectify_create_calib": (C.c_int, [C.POINTER(Calib), C.POINTER(Rectification), C.c_int, C.c_int, C.c_int, C.c_int,
                                            C.c_int, C.c_int, C.POINTER(vp)]),
    "rtdm_objects_create": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(vp)]),
    "rtdm_objects_destroy": (None, [vp]),
    "rtdm_objects_detect": (C.c_int, [vp, u8p, sz, C.POINTER(HsvRange), C.c_int, C.c_int, u8p, sz, C.POINTER(Region), C.c_int,
                                      C.POINTER(C.c_int), C.POINTER(Region)]),
    "rtdm_estimate_frame": (C.c_int, [vp, vp, vp, u8p, sz, u8p, sz, C.POINTER(C.c_double), C.POINTER(HsvRange), C.c_int, C.c_int,
                                      C.c_double, C.POINTER(Region), C.POINTER(C.c_double), C.POINTER(C.c_int), C.c_int,
                                      C.POINTER(C.c_int), i16p, sz]),
    "rtdm_objects_create_batch": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(vp)]),
    "rtdm_objects_detect_device": (C.c_int, [vp, C.c_int, u8p, sz, sz, C.POINTER(HsvRange), C.POINTER(C.c_int), C.c_int, C.c_int,
                                             C.c_int, C.c_int, u8p, sz, sz, vp, C.c_int, vp, vp, vp]),
    "rtdm_objects_detect_batch": (C.c_int, [vp, C.c_int, u8p, sz, sz, C.POINTER(HsvRange), C.POINTER(C.c_int), C.c_int, C.c_int,
                                            C.c_int, C.c_int, u8p, sz, sz, vp, C.c_int, vp, vp]),
    "rtdm_estimate_frame_classes": (C.c_int, [vp, vp, vp, u8p, sz, u8p, sz, C.POINTER(C.c_double), C.POINTER(HsvRange),
                                              C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, vp,
                                              C.POINTER(C.c_double), C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int), i16p, sz]),
    "rtdm_objects_detect_labels_device": (C.c_int, [vp, C.c_int, u8p, sz, sz, C.POINTER(HsvRange), C.POINTER(C.c_int), C.c_int, C.c_int,
                                                    C.c_int, C.c_int, u8p, sz, sz, vp, C.c_int, vp, vp, vp, sz, sz, vp, vp]),
    "rtdm_objects_detect_labels_batch": (C.c_int, [vp, C.c_int, u8p, sz, sz, C.POINTER(HsvRange), C.POINTER(C.c_int), C.c_int, C.c_int,
                                                   C.c_int, C.c_int, u8p, sz, sz, vp, C.c_int, vp, vp, vp, sz, sz, vp]),
    "rtdm_depth_objects_labels_device": (C.c_int, [C.c_int, C.c_int, i16p, sz, sz, C.c_int, C.c_int, C.POINTER(C.c_double), vp, sz, sz,
                                                   C.c_int, vp, C.c_int, vp, C.c_double, vp, vp, vp, sz, vp]),
    "rtdm_estimator_set_own_pixels": (C.c_int, [vp, C.c_int]),
    "rtdm_estimator_get_own_pixels": (C.c_int, [vp, C.POINTER(C.c_int)]),
    "rtdm_estimator_set_device_roi": (C.c_int, [vp, C.c_int]),
    "rtdm_estimator_get_device_roi": (C.c_int, [vp, C.POINTER(C.c_int)]),
    "rtdm_depth_objects_workspace_bytes": (sz, [C.c_int, C.c_int, C.c_int]),
    "rtdm_depth_objects_device": (C.c_int, [C.c_int, C.c_int, i16p, sz, sz, C.c_int, C.c_int, C.POINTER(C.c_double), u8p, sz, sz,
                                            C.c_int, vp, C.c_int, vp, C.c_double, vp, vp, vp, sz, vp]),
    "rtdm_estimator_create": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.POINTER(vp)]),
    "rtdm_estimator_destroy": (None, [vp]),
    "rtdm_estimate_batch": (C.c_int, [vp, C.c_int, u8p, sz, sz, u8p, sz, sz, C.POINTER(C.c_double), C.POINTER(HsvRange),
                                      C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, vp, vp, vp, vp, i16p, sz, sz]),
    "rtdm_estimate_batch_device": (C.c_int, [vp, C.c_int, u8p, sz, sz, u8p, sz, sz, C.POINTER(C.c_double), C.POINTER(HsvRange),
                                             C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, vp, vp, vp, vp, i16p,
                                             sz, sz, vp]),
    "rtdm_measure_default_params": (None, [C.POINTER(MeasureParams)]),
    "rtdm_objects_measure_workspace_bytes": (sz, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "rtdm_objects_measure_device": (C.c_int, [C.c_int, C.POINTER(MeasureParams), C.c_int, i16p, sz, sz, C.c_int, C.c_int,
                                              C.POINTER(C.c_double), vp, sz, sz, C.c_int, C.c_int, vp, C.c_int, vp, vp, vp, sz, vp]),
    "rtdm_estimate_batch_measured": (C.c_int, [vp, C.c_int, u8p, sz, sz, u8p, sz, sz, C.POINTER(C.c_double), C.POINTER(HsvRange),
                                               C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, vp, vp, vp, vp, i16p,
                                               sz, sz, C.POINTER(MeasureParams), vp]),
    "rtdm_estimate_batch_measured_device": (C.c_int, [vp, C.c_int, u8p, sz, sz, u8p, sz, sz, C.POINTER(C.c_double), C.POINTER(HsvRange),
                                                      C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, vp, vp, vp, vp,
                                                      i16p, sz, sz, vp, C.POINTER(MeasureParams), vp]),
    "rtdm_wls_params_for_bm": (C.c_int, [C.POINTER(BMParams), C.POINTER(WLSParams)]),
    "rtdm_wls_params_for_sgm": (C.c_int, [C.POINTER(SGMParams), C.POINTER(WLSParams)]),
    "rtdm_bm_right_params": (C.c_int, [C.POINTER(BMParams), C.POINTER(BMParams)]),
    "rtdm_sgm_right_params": (C.c_int, [C.POINTER(SGMParams), C.POINTER(SGMParams)]),
    "rtdm_wls_create": (C.c_int, [C.POINTER(WLSParams), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(vp)]),
    "rtdm_wls_destroy": (None, [vp]),
    "rtdm_wls_set_params": (C.c_int, [vp, C.POINTER(WLSParams)]),
    "rtdm_wls_get_params": (C.c_int, [vp, C.POINTER(WLSParams)]),
    "rtdm_wls_filter": (C.c_int, [vp, i16p, sz, i16p, sz, u8p, sz, C.c_int, C.c_int, C.c_int, i16p, sz, vp, sz, vp, sz]),
    "rtdm_wls_filter_device": (C.c_int, [vp, C.c_int, i16p, sz, sz, i16p, sz, sz, u8p, sz, sz, C.c_int, C.c_int, C.c_int,
                                         i16p, sz, sz, vp, sz, sz, vp, sz, sz, vp]),
    "rtdm_bm_compute_filtered": (C.c_int, [vp, vp, vp, u8p, sz, u8p, sz, C.c_int, C.c_int, i16p, sz, i16p, sz]),
    "rtdm_xyz_default_params": (None, [C.POINTER(XYZParams), C.POINTER(C.c_double), C.c_int]),
    "rtdm_xyz_create": (C.c_int, [C.POINTER(XYZParams), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(vp)]),
    "rtdm_xyz_destroy": (None, [vp]),
    "rtdm_xyz_set_params": (C.c_int, [vp, C.POINTER(XYZParams)]),
    "rtdm_xyz_get_params": (C.c_int, [vp, C.POINTER(XYZParams)]),
    "rtdm_xyz_map": (C.c_int, [vp, i16p, sz, C.c_int, C.c_int, vp, sz, vp, sz]),
    "rtdm_xyz_map_device": (C.c_int, [vp, C.c_int, i16p, sz, sz, C.c_int, C.c_int, vp, sz, sz, vp, sz, sz, vp]),
    "rtdm_xyz_cloud": (C.c_int, [vp, i16p, sz, u8p, sz, C.c_int, u8p, sz, C.c_int, C.c_int, vp, C.c_int, C.POINTER(C.c_int)]),
    "rtdm_xyz_cloud_device": (C.c_int, [vp, C.c_int, i16p, sz, sz, u8p, sz, sz, C.c_int, u8p, sz, sz, C.c_int, C.c_int,
                                        vp, sz, C.c_int, vp, vp]),
    "rtdm_bm_compute_cloud": (C.c_int, [vp, vp, u8p, sz, u8p, sz, C.c_int, C.c_int, u8p, sz, C.c_int, u8p, sz, vp, C.c_int,
                                        C.POINTER(C.c_int), i16p, sz]),
    "rtdm_mjpeg_probe": (C.c_int, [u8p, sz, C.POINTER(MJPEGInfo)]),
    "rtdm_mjpeg_create": (C.c_int, [C.c_int, C.c_int, C.c_int, sz, C.c_int, C.POINTER(vp)]),
    "rtdm_mjpeg_destroy": (None, [vp]),
    "rtdm_mjpeg_decode": (C.c_int, [vp, u8p, sz, C.c_int, C.c_int, u8p, sz]),
    "rtdm_mjpeg_decode_batch_device": (C.c_int, [vp, C.c_int, C.POINTER(C.c_void_p), C.POINTER(sz), C.c_int, C.c_int, u8p,
                                                 sz, sz, vp, vp]),
    "rtdm_bm_compute_mjpeg": (C.c_int, [vp, vp, vp, u8p, sz, u8p, sz, C.c_int, C.c_int, i16p, sz]),
    "rtdm_mjpeg_set_split": (C.c_int, [vp, C.c_int]),
    "rtdm_mjpeg_get_split": (C.c_int, [vp, C.POINTER(C.c_int)]),
    "rtdm_mjpeg_get_split_stats": (C.c_int, [vp, C.POINTER(C.c_long), C.POINTER(C.c_long), C.POINTER(C.c_int)]),
    "rtdm_synth_pairs_device": (C.c_int, [C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, u8p, u8p,
                                          sz, sz, C.c_int, vp]),
}
EXPORTS = tuple(SIGNATURES)

_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("HIP extension %s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(there is no CPU fallback)" % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = res, args
    _lib = L
    return L


def check(status, where):
    if status != RTDM_OK:
        detail = lib().rtdm_last_hip_error().decode() if status == -4 else ""
        raise RtdmError(status, where, detail)


def make_params(preFilterCap=31, blockSize=13, minDisparity=0, numDisparities=64, textureThreshold=10,
                uniquenessRatio=10, speckleWindowSize=100, speckleRange=32, disp12MaxDiff=1, legacy_right_clamp=0):
    """Defaults are the reference's literals (main.cpp:134-135)."""
    return BMParams(preFilterCap, blockSize, minDisparity, numDisparities, textureThreshold,
                    uniquenessRatio, speckleWindowSize, speckleRange, disp12MaxDiff, legacy_right_clamp)
