"""Host-side mirror of the reference's plugin interfaces, for tests and bench.py.

``HIPMatcher`` mirrors ``BlockMatcher`` (include/stereo-matcher/stereo-matcher.h:13-19) with the
constructor shape of ``SWMatcherKonolige`` (include/stereo-matcher/bm-sw.h:28-30):
``compute(left, right) -> disp``, ``setROI1``, ``setROI2``.  ``HIPMorphologicalFilter`` mirrors
``VideoFilterDevice`` (include/filter/filter.h:13-37): ``run``, ``getVideoInBuffer`` ...
The C++ adapter that actually plugs into the reference is rt-depth-map_amd/host/bm-hip.{h,cpp}; both
are thin shells over the same C ABI (include/rtdm.h).
"""
import ctypes as C

import numpy as np

from . import binding as B

PREFILTER_NORMALIZED_RESPONSE, PREFILTER_XSOBEL = B.PREFILTER_NORMALIZED_RESPONSE, B.PREFILTER_XSOBEL


class HIPMatcher:
    """numOfDisparities: any multiple of 16 with minDisparity + numOfDisparities <= 2047 (up to 4080), any odd blockSize
    5..255 -- the parameters go to rtdm_bm_create unchanged; only frames wider than 4096 are refused.
    preFilterType (PREFILTER_XSOBEL, PREFILTER_NORMALIZED_RESPONSE) and preFilterSize (odd, 5..255) are cv::StereoBM's;
    they go through rtdm_bm_set_prefilter, at construction and by setPreFilterType / setPreFilterSize."""
    def __init__(self, roi1=None, roi2=None, preFilterCap=31, blockSize=13, minDisparity=0, textureThreshold=10,
                 numOfDisparities=64, maxDisparity=None, uniquenessRatio=10, speckleWindowSize=100,
                 speckleRange=32, disp12MaxDiff=1, width=1280, height=720, max_batch=1, device=0, legacy_right_clamp=0,
                 preFilterType=PREFILTER_XSOBEL, preFilterSize=9):
        # roi1/roi2/maxDisparity are accepted and ignored, exactly like bm-sw.cpp:12-26
        self._h = C.c_void_p()
        self.params = B.make_params(preFilterCap, blockSize, minDisparity, numOfDisparities, textureThreshold,
                                    uniquenessRatio, speckleWindowSize, speckleRange, disp12MaxDiff, legacy_right_clamp)
        self.width, self.height, self.max_batch, self.device = width, height, max_batch, device
        B.check(B.lib().rtdm_bm_create(C.byref(self.params), width, height, max_batch, device, C.byref(self._h)),
                "rtdm_bm_create")
        if (preFilterType, preFilterSize) != (PREFILTER_XSOBEL, 9):
            try:
                self._set_prefilter(preFilterType, preFilterSize)
            except B.RtdmError:
                self.close()
                raise

    def _set_prefilter(self, preFilterType, preFilterSize):
        B.check(B.lib().rtdm_bm_set_prefilter(self._h, int(preFilterType), int(preFilterSize)), "rtdm_bm_set_prefilter")

    def _get_prefilter(self):
        t, s = C.c_int(), C.c_int()
        B.check(B.lib().rtdm_bm_get_prefilter(self._h, C.byref(t), C.byref(s)), "rtdm_bm_get_prefilter")
        return t.value, s.value

    def setPreFilterType(self, preFilterType):
        """cv::StereoBM::setPreFilterType: applies from the next compute call."""
        self._set_prefilter(preFilterType, self._get_prefilter()[1])

    def setPreFilterSize(self, preFilterSize):
        """cv::StereoBM::setPreFilterSize (odd, 5..255; only NORMALIZED_RESPONSE reads it): applies from the next compute call."""
        self._set_prefilter(self._get_prefilter()[0], preFilterSize)

    def getPreFilterType(self):
        return self._get_prefilter()[0]

    def getPreFilterSize(self):
        return self._get_prefilter()[1]

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            try:
                B.lib().rtdm_bm_destroy(self._h)
            except (TypeError, AttributeError):       # interpreter shutdown: the module globals are already gone
                pass
            self._h = None

    __del__ = close

    def setROI1(self, roi):
        B.check(B.lib().rtdm_bm_set_roi(self._h, 1, *[int(v) for v in roi]), "rtdm_bm_set_roi")

    def setROI2(self, roi):
        B.check(B.lib().rtdm_bm_set_roi(self._h, 2, *[int(v) for v in roi]), "rtdm_bm_set_roi")

    @property
    def filtered(self):
        return (self.params.minDisparity - 1) * 16

    def compute(self, left, right, out=None):
        """left/right: 2-D uint8 numpy arrays (row stride free, column stride 1) -> int16 HxW (x16).
        out: an int16 HxW array (column stride 1) to write into -- what a caller that keeps its cv::Mat does."""
        assert left.dtype == np.uint8 and right.dtype == np.uint8 and left.shape == right.shape
        assert left.ndim == 2 and left.strides[1] == 1 and right.strides[1] == 1
        H, W = left.shape
        disp = np.empty((H, W), np.int16) if out is None else out
        assert disp.dtype == np.int16 and disp.shape == (H, W) and disp.strides[1] == 2
        B.check(B.lib().rtdm_bm_compute(self._h, left.ctypes.data, left.strides[0], right.ctypes.data,
                                        right.strides[0], W, H, disp.ctypes.data, disp.strides[0]), "rtdm_bm_compute")
        return disp

    def compute_depth(self, left, right, Q, mask, regions, calibration_unit=25.0, want_disp=False):
        """estimator.cpp:56,75-77 in one call: match, /= 16, reproject with Q, mean Z per region under `mask`.
        Returns (mean_cm[n], counts[n]) and, if want_disp, the x16 disparity map as well."""
        assert left.dtype == np.uint8 and right.dtype == np.uint8 and mask.dtype == np.uint8 and left.shape == right.shape == mask.shape
        H, W = left.shape
        q = np.ascontiguousarray(Q, np.float64).reshape(16)
        n = len(regions)
        reg = (B.Region * max(n, 1))(*[B.Region(*[int(v) for v in r]) for r in regions])
        mean = np.zeros(n, np.float64); cnt = np.zeros(n, np.int32)
        disp = np.empty((H, W), np.int16) if want_disp else None
        B.check(B.lib().rtdm_bm_compute_depth(
            self._h, left.ctypes.data, left.strides[0], right.ctypes.data, right.strides[0], W, H,
            q.ctypes.data_as(C.POINTER(C.c_double)), mask.ctypes.data, mask.strides[0], reg, n, calibration_unit,
            mean.ctypes.data_as(C.POINTER(C.c_double)), cnt.ctypes.data_as(C.POINTER(C.c_int)),
            disp.ctypes.data if want_disp else None, W * 2), "rtdm_bm_compute_depth")
        return (mean, cnt, disp) if want_disp else (mean, cnt)

    def compute_batch(self, left, right, out=None):
        """left/right: uint8 [n, H, W] host arrays (frame and row strides free, column stride 1: views of wider planes are
        passed as they are) -> int16 [n, H, W] (out: an int16 [n, H, W] array, column stride 2 bytes, to write into).
        Page-locked arrays (hipHostMalloc / torch pin_memory) move by DMA beside the compute."""
        def plane(a):
            a = np.asarray(a)
            ok = a.dtype == np.uint8 and a.ndim == 3 and a.strides[2] == 1 and a.strides[1] >= a.shape[2] and a.strides[0] >= 0
            return a if ok else np.ascontiguousarray(a, np.uint8)
        left, right = plane(left), plane(right)
        if left.strides != right.strides:
            left, right = np.ascontiguousarray(left), np.ascontiguousarray(right)
        n, H, W = left.shape
        assert right.shape == left.shape
        disp = np.empty((n, H, W), np.int16) if out is None else out
        assert disp.dtype == np.int16 and disp.shape == (n, H, W) and disp.strides[2] == 2 and disp.strides[1] >= W * 2
        B.check(B.lib().rtdm_bm_compute_batch(self._h, n, left.ctypes.data, right.ctypes.data, left.strides[1], left.strides[0], W, H,
                                              disp.ctypes.data, disp.strides[1], disp.strides[0]), "rtdm_bm_compute_batch")
        return disp

    def compute_device(self, d_left, d_right, d_disp, stream=None):
        """torch CUDA tensors: uint8 [n,H,W] x2, int16 [n,H,W]; enqueued on ``stream`` (a raw
        hipStream_t value, e.g. torch.cuda.current_stream().cuda_stream), not synchronised."""
        n, H, W = d_left.shape
        assert d_left.is_contiguous() and d_right.is_contiguous() and d_disp.is_contiguous()
        B.check(B.lib().rtdm_bm_compute_device(self._h, n, d_left.data_ptr(), d_right.data_ptr(), W, W * H, W, H,
                                               d_disp.data_ptr(), W * 2, W * H * 2, stream), "rtdm_bm_compute_device")

    def synchronize(self):
        B.check(B.lib().rtdm_bm_synchronize(self._h), "rtdm_bm_synchronize")

    def set_profiling(self, on):
        B.check(B.lib().rtdm_bm_set_profiling(self._h, int(bool(on))), "rtdm_bm_set_profiling")

    def reset_stage_times(self):
        B.check(B.lib().rtdm_bm_reset_stage_times(self._h), "rtdm_bm_reset_stage_times")

    def stage_times(self):
        out = {}
        for i, name in enumerate(B.STAGES):
            ms, nl, nf = C.c_double(), C.c_long(), C.c_long()
            B.check(B.lib().rtdm_bm_get_stage_time(self._h, i, C.byref(ms), C.byref(nl), C.byref(nf)), "get_stage_time")
            out[name] = dict(total_ms=ms.value, launches=nl.value, frames=nf.value)
        return out

    @property
    def search_variant(self):
        return B.lib().rtdm_bm_search_variant(self._h).decode()

    def tuner_stats(self):
        """(batch shapes whose strip count was measured, extra search launches that took) -- rtdm_bm_get_tuner_stats."""
        a, b = C.c_long(), C.c_long()
        B.check(B.lib().rtdm_bm_get_tuner_stats(self._h, C.byref(a), C.byref(b)), "rtdm_bm_get_tuner_stats")
        return a.value, b.value


class HIPSemiGlobalMatcher:
    """BlockMatcher over rtdm_sgm_*; constructor shape of SWSemiGlobalMatcher
    (include/stereo-matcher/sgbm-sw.h:27-28): blockSize, minDisparity, numOfDisparities, uniquenessRatio,
    speckleWindowSize, speckleRange, disp12MaxDiff; P1/P2 are the literals of sgbm-sw.cpp:17-18.  numOfDisparities is
    any multiple of 16, as in cv::StereoSGBM (above 256 the path passes run on the wide-line kernel); the library checks it.
    preFilterCap is cv::StereoSGBM's (0 .. 127, setPreFilterCap); compute / compute_device take gray (H x W) or
    interleaved colour (H x W x 3) uint8 frames, as cv::StereoSGBM::compute takes CV_8UC1 and CV_8UC3.
    mode is cv::StereoSGBM::setMode's value (MODE_SGBM, MODE_HH, MODE_HH4; MODE_SGBM_3WAY is refused by the library with
    RTDM_ERR_UNSUPPORTED); paths names the same thing by its direction count (5, 8, 4) and defaults to 8."""

    MODE_SGBM, MODE_HH, MODE_SGBM_3WAY, MODE_HH4 = 0, 1, 2, 3          # cv::StereoSGBM's values
    _MODE_PATHS = {MODE_SGBM: 5, MODE_HH: 8, MODE_SGBM_3WAY: 3, MODE_HH4: 4}

    def __init__(self, blockSize=5, minDisparity=0, numOfDisparities=128, uniquenessRatio=10, speckleWindowSize=100,
                 speckleRange=32, disp12MaxDiff=1, P1=600, P2=2400, width=1280, height=720, max_batch=1, device=0, paths=None,
                 preFilterCap=0, mode=None):
        # paths: 5 = cv::StereoSGBM's default MODE_SGBM (what sgbm-sw.cpp:15 creates), 8 = MODE_HH (BASELINE config 5),
        # 4 = MODE_HH4 (the two horizontal and the two vertical directions)
        if mode is not None:
            if mode not in self._MODE_PATHS:
                raise ValueError("mode must be MODE_SGBM (0), MODE_HH (1), MODE_SGBM_3WAY (2) or MODE_HH4 (3); got %r" % (mode,))
            if paths is not None and paths != self._MODE_PATHS[mode]:
                raise ValueError("mode=%d means paths=%d; got paths=%d" % (mode, self._MODE_PATHS[mode], paths))
            paths = self._MODE_PATHS[mode]
        elif paths is None:
            paths = 8
        self._h = C.c_void_p()
        self.params = B.SGMParams(blockSize, minDisparity, numOfDisparities, P1, P2, uniquenessRatio, speckleWindowSize,
                                  speckleRange, disp12MaxDiff, paths)
        self.width, self.height, self.max_batch, self.device = width, height, max_batch, device
        B.check(B.lib().rtdm_sgm_create(C.byref(self.params), width, height, max_batch, device, C.byref(self._h)),
                "rtdm_sgm_create")
        self.preFilterCap = 0
        if preFilterCap:
            try:
                self.setPreFilterCap(preFilterCap)
            except B.RtdmError:
                self.close()
                raise

    def setPreFilterCap(self, preFilterCap):
        """cv::StereoSGBM::setPreFilterCap: applies from the next compute call; >= 128 is refused (RTDM_ERR_UNSUPPORTED)."""
        B.check(B.lib().rtdm_sgm_set_prefilter_cap(self._h, int(preFilterCap)), "rtdm_sgm_set_prefilter_cap")
        self.preFilterCap = int(preFilterCap)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            try:
                B.lib().rtdm_sgm_destroy(self._h)
            except (TypeError, AttributeError):
                pass
            self._h = None

    __del__ = close

    def setROI1(self, roi):     # no-ops in the reference (sgbm-sw.h:32-33)
        pass

    def setROI2(self, roi):
        pass

    @property
    def filtered(self):
        return (self.params.minDisparity - 1) * 16

    @property
    def mode(self):
        """cv::StereoSGBM::getMode of this matcher's direction set"""
        return {v: k for k, v in self._MODE_PATHS.items()}[self.params.paths]

    @staticmethod
    def _channels(shape, lead):
        """channel count of a gray (lead + (H, W)) or colour (lead + (H, W, 3)) frame shape"""
        if len(shape) == lead + 2:
            return 1
        if len(shape) == lead + 3 and shape[-1] == 3:
            return 3
        raise ValueError("StereoSGBM frames are %s x H x W (gray) or %s x H x W x 3 (interleaved colour) uint8; got shape %s"
                         % (("n",) * lead or "", ("n",) * lead or "", tuple(shape)))

    def compute(self, left, right):
        if not isinstance(left, np.ndarray) or not isinstance(right, np.ndarray):
            raise TypeError("compute takes numpy arrays")
        if left.dtype != np.uint8 or right.dtype != np.uint8:
            raise TypeError("StereoSGBM frames are uint8; got %s and %s" % (left.dtype, right.dtype))
        if left.shape != right.shape:
            raise ValueError("left and right frames differ in shape: %s vs %s" % (left.shape, right.shape))
        cn = self._channels(left.shape, 0)
        H, W = left.shape[:2]
        for a in (left, right):
            if a.strides[1] != cn or (cn == 3 and a.strides[2] != 1):
                raise ValueError("frame rows must be contiguous (pixels %d bytes apart); got strides %s" % (cn, a.strides))
        disp = np.empty((H, W), np.int16)
        B.check(B.lib().rtdm_sgm_compute_cn(self._h, cn, left.ctypes.data, left.strides[0], right.ctypes.data,
                                            right.strides[0], W, H, disp.ctypes.data, W * 2), "rtdm_sgm_compute_cn")
        return disp

    def pass_stats(self):
        """(row-synchronous sweeps launched so far, whether one has given up) -- rtdm_sgm_get_pass_stats"""
        sw, gu = C.c_long(0), C.c_int(0)
        B.check(B.lib().rtdm_sgm_get_pass_stats(self._h, C.byref(sw), C.byref(gu)), "rtdm_sgm_get_pass_stats")
        return sw.value, bool(gu.value)

    @property
    def path_variant(self):
        """the path-pass form of the last call: "sweep", "vert", "half", "wide_w1", "wide_w4" -- rtdm_sgm_path_variant"""
        return B.lib().rtdm_sgm_path_variant(self._h).decode()

    def compute_device(self, d_left, d_right, d_disp, stream=None):
        """d_left, d_right: contiguous (n, H, W) or (n, H, W, 3) uint8 device tensors; d_disp: (n, H, W) int16."""
        if tuple(d_left.shape) != tuple(d_right.shape):
            raise ValueError("left and right frames differ in shape: %s vs %s" % (tuple(d_left.shape), tuple(d_right.shape)))
        cn = self._channels(tuple(d_left.shape), 1)
        n, H, W = d_left.shape[:3]
        B.check(B.lib().rtdm_sgm_compute_device_cn(self._h, cn, n, d_left.data_ptr(), d_right.data_ptr(), W * cn, W * H * cn,
                                                   W, H, d_disp.data_ptr(), W * 2, W * H * 2, stream),
                "rtdm_sgm_compute_device_cn")


def _wls_plane(a, dtype, name, shape=None):
    if not isinstance(a, np.ndarray):
        raise TypeError("%s must be a numpy array" % name)
    if a.dtype != dtype:
        raise ValueError("%s must be %s; got %s" % (name, np.dtype(dtype).name, a.dtype))
    if shape is not None and a.shape[:2] != shape:
        raise ValueError("%s has shape %s; expected %s" % (name, a.shape, shape))
    if a.strides[1] != a.itemsize * (a.shape[2] if a.ndim == 3 else 1) or (a.ndim == 3 and a.strides[2] != a.itemsize):
        raise ValueError("%s rows must be contiguous; got strides %s" % (name, a.strides))
    return a


def create_right_matcher(m):
    """cv::ximgproc::createRightMatcher (W1): the same matcher searching right against left; call it as compute(right, left)."""
    if isinstance(m, HIPMatcher):
        rp = B.BMParams()
        B.check(B.lib().rtdm_bm_right_params(C.byref(m.params), C.byref(rp)), "rtdm_bm_right_params")
        return HIPMatcher(preFilterCap=rp.preFilterCap, blockSize=rp.blockSize, minDisparity=rp.minDisparity,
                          textureThreshold=rp.textureThreshold, numOfDisparities=rp.numDisparities,
                          uniquenessRatio=rp.uniquenessRatio, speckleWindowSize=rp.speckleWindowSize,
                          speckleRange=rp.speckleRange, disp12MaxDiff=rp.disp12MaxDiff, width=m.width, height=m.height,
                          max_batch=m.max_batch, device=m.device, legacy_right_clamp=rp.legacy_right_clamp,
                          preFilterType=m.getPreFilterType(), preFilterSize=m.getPreFilterSize())
    if isinstance(m, HIPSemiGlobalMatcher):
        rp = B.SGMParams()
        B.check(B.lib().rtdm_sgm_right_params(C.byref(m.params), C.byref(rp)), "rtdm_sgm_right_params")
        return HIPSemiGlobalMatcher(blockSize=rp.blockSize, minDisparity=rp.minDisparity, numOfDisparities=rp.numDisparities,
                                    uniquenessRatio=rp.uniquenessRatio, speckleWindowSize=rp.speckleWindowSize,
                                    speckleRange=rp.speckleRange, disp12MaxDiff=rp.disp12MaxDiff, P1=rp.P1, P2=rp.P2,
                                    width=m.width, height=m.height, max_batch=m.max_batch, device=m.device, paths=rp.paths,
                                    preFilterCap=m.preFilterCap)
    raise ValueError("create_right_matcher takes a HIPMatcher or a HIPSemiGlobalMatcher; got %s" % type(m).__name__)


def wls_params_for(m):
    """W2: the rtdm_wls_params createDisparityWLSFilter derives from a left HIPMatcher / HIPSemiGlobalMatcher."""
    p = B.WLSParams()
    if isinstance(m, HIPMatcher):
        B.check(B.lib().rtdm_wls_params_for_bm(C.byref(m.params), C.byref(p)), "rtdm_wls_params_for_bm")
    elif isinstance(m, HIPSemiGlobalMatcher):
        B.check(B.lib().rtdm_wls_params_for_sgm(C.byref(m.params), C.byref(p)), "rtdm_wls_params_for_sgm")
    else:
        raise ValueError("wls_params_for takes a HIPMatcher or a HIPSemiGlobalMatcher; got %s" % type(m).__name__)
    return p


def create_disparity_wls_filter(m, max_batch=None):
    """cv::ximgproc::createDisparityWLSFilter(matcher_left) for frames of the matcher's size."""
    return HIPDisparityWLSFilter(wls_params_for(m), m.width, m.height, max_batch=max_batch or m.max_batch, device=m.device)


class HIPDisparityWLSFilter:
    """cv::ximgproc::DisparityWLSFilter over rtdm_wls_* (rules W1-W8).  params: a binding.WLSParams
    (wls_params_for / create_disparity_wls_filter make it from a matcher).  filter(disparity_map_left, left_view, filtered,
    disparity_map_right) has ximgproc's call shape; the filtered map is int16 x16 with the left matcher's invalid value."""

    def __init__(self, params, width, height, max_batch=1, device=0):
        self._h = C.c_void_p()
        self.params = B.WLSParams()
        C.memmove(C.byref(self.params), C.byref(params), C.sizeof(B.WLSParams))
        self.width, self.height, self.max_batch, self.device = width, height, max_batch, device
        self.confidence_map = None
        B.check(B.lib().rtdm_wls_create(C.byref(self.params), width, height, max_batch, device, C.byref(self._h)), "rtdm_wls_create")

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            try:
                B.lib().rtdm_wls_destroy(self._h)
            except (TypeError, AttributeError):
                pass
            self._h = None

    __del__ = close

    def _set(self, **kw):
        p = B.WLSParams()
        C.memmove(C.byref(p), C.byref(self.params), C.sizeof(B.WLSParams))
        for k, v in kw.items():
            setattr(p, k, v)
        B.check(B.lib().rtdm_wls_set_params(self._h, C.byref(p)), "rtdm_wls_set_params")
        self.params = p

    def setLambda(self, v):
        self._set(lambda_=float(v))

    def getLambda(self):
        return self.params.lambda_

    def setSigmaColor(self, v):
        self._set(sigma_color=float(v))

    def getSigmaColor(self):
        return self.params.sigma_color

    def setLRCthresh(self, v):
        self._set(lrc_thresh=int(v))

    def getLRCthresh(self):
        return self.params.lrc_thresh

    def setDepthDiscontinuityRadius(self, v):
        self._set(depth_discontinuity_radius=int(v))

    def getDepthDiscontinuityRadius(self):
        return self.params.depth_discontinuity_radius

    def getConfidenceMap(self):
        """C of the last host call (float32, 0 / 255; 0 outside the ROI)."""
        return self.confidence_map

    def getROI(self, width=None, height=None):
        """(x, y, w, h) of the valid ROI for a frame of this size (W2); (0, 0, 0, 0) when it is empty."""
        W = self.width if width is None else width
        H = self.height if height is None else height
        p = self.params
        w, h = W - p.roi_left - p.roi_right, H - p.roi_top - p.roi_bottom
        return (p.roi_left, p.roi_top, w, h) if w > 0 and h > 0 else (0, 0, 0, 0)

    @property
    def invalid(self):
        return (self.params.min_disparity - 1) * 16

    def filter(self, disparity_map_left, left_view, filtered=None, disparity_map_right=None, want_float=False):
        """-> int16 H x W (written into `filtered` if given); with want_float also the float32 F1 / F2 map."""
        dl = _wls_plane(disparity_map_left, np.int16, "disparity_map_left")
        if dl.ndim != 2:
            raise ValueError("disparity_map_left must be H x W; got shape %s" % (dl.shape,))
        H, W = dl.shape
        dr = None
        if self.params.use_confidence:
            if disparity_map_right is None:
                raise ValueError("this filter uses a confidence map: disparity_map_right is required")
            dr = _wls_plane(disparity_map_right, np.int16, "disparity_map_right", (H, W))
        g = _wls_plane(left_view, np.uint8, "left_view", (H, W))
        cn = 1 if g.ndim == 2 else g.shape[2]
        out = np.empty((H, W), np.int16) if filtered is None else _wls_plane(filtered, np.int16, "filtered", (H, W))
        conf = np.empty((H, W), np.float32)
        fl = np.empty((H, W), np.float32) if want_float else None
        B.check(B.lib().rtdm_wls_filter(self._h, dl.ctypes.data, dl.strides[0], dr.ctypes.data if dr is not None else None,
                                        dr.strides[0] if dr is not None else 0, g.ctypes.data, g.strides[0], cn, W, H,
                                        out.ctypes.data, out.strides[0], conf.ctypes.data, conf.strides[0],
                                        fl.ctypes.data if want_float else None, W * 4), "rtdm_wls_filter")
        self.confidence_map = conf
        return (out, fl) if want_float else out

    def filter_device(self, d_left, d_right, d_guide, d_out, d_conf=None, d_filtered=None, stream=None):
        """Contiguous torch device tensors: int16 [n,H,W] maps (d_right may be None without confidence), uint8 [n,H,W] or
        [n,H,W,3] guide, int16 [n,H,W] out, optional float32 [n,H,W] confidence / filtered.  Enqueued on `stream`, not
        synchronised."""
        if d_left.dim() != 3:
            raise ValueError("d_left must be n x H x W; got %s" % (tuple(d_left.shape),))
        n, H, W = d_left.shape
        if d_guide.dim() not in (3, 4) or tuple(d_guide.shape[:3]) != (n, H, W):
            raise ValueError("d_guide must be n x H x W or n x H x W x 3; got %s" % (tuple(d_guide.shape),))
        cn = 1 if d_guide.dim() == 3 else d_guide.shape[3]
        for t in (d_left, d_right, d_guide, d_out, d_conf, d_filtered):
            if t is not None and not t.is_contiguous():
                raise ValueError("device tensors must be contiguous")
        ptr = lambda t: t.data_ptr() if t is not None else None
        B.check(B.lib().rtdm_wls_filter_device(self._h, n, d_left.data_ptr(), W * 2, W * H * 2, ptr(d_right), W * 2, W * H * 2,
                                               d_guide.data_ptr(), W * cn, W * H * cn, cn, W, H, d_out.data_ptr(), W * 2,
                                               W * H * 2, ptr(d_conf), W * 4, W * H * 4, ptr(d_filtered), W * 4, W * H * 4, stream),
                "rtdm_wls_filter_device")

    def compute_filtered(self, left_matcher, right_matcher, left, right, want_raw=False):
        """estimator.cpp:56-61 in one call (rtdm_bm_compute_filtered): gray pair in, filtered x16 map out (and the left
        matcher's raw map with want_raw).  right_matcher: create_right_matcher(left_matcher)."""
        if not isinstance(left_matcher, HIPMatcher) or (right_matcher is not None and not isinstance(right_matcher, HIPMatcher)):
            raise ValueError("compute_filtered runs StereoBM handles (HIPMatcher)")
        l = _wls_plane(left, np.uint8, "left")
        r = _wls_plane(right, np.uint8, "right", l.shape)
        if l.ndim != 2:
            raise ValueError("compute_filtered takes gray frames")
        H, W = l.shape
        out = np.empty((H, W), np.int16)
        raw = np.empty((H, W), np.int16) if want_raw else None
        B.check(B.lib().rtdm_bm_compute_filtered(left_matcher._h, right_matcher._h if right_matcher is not None else None, self._h,
                                                 l.ctypes.data, l.strides[0], r.ctypes.data, r.strides[0], W, H,
                                                 out.ctypes.data, W * 2, raw.ctypes.data if want_raw else None, W * 2),
                "rtdm_bm_compute_filtered")
        return (out, raw) if want_raw else out


POINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("r", "u1"), ("g", "u1"), ("b", "u1"), ("a", "u1")])   # rtdm_point
XYZ_FIXED16, XYZ_ROUNDED = B.XYZ_FIXED16, B.XYZ_ROUNDED


class HIPReprojector:
    """cv::reprojectImageTo3D (estimator.cpp:76) and the point cloud of the pixels calc_depth keeps (estimator.cpp:235) over
    rtdm_xyz_* (rules X1-X8).  Q: 4x4; mode: XYZ_ROUNDED (the reference's `left_disp /= 16.`) or
    XYZ_FIXED16 (d = disp / 16.0, sub-pixel); min_disparity: the matcher's.  Disparity maps are the matchers' int16 x16 maps."""

    def __init__(self, Q, width, height, min_disparity=0, mode=XYZ_ROUNDED, handleMissingValues=True, max_z=1e4, max_batch=1,
                 device=0):
        q = np.asarray(Q, np.float64)
        if q.size != 16:
            raise ValueError("Q must have 16 entries (4 x 4); got shape %s" % (q.shape,))
        self._h = C.c_void_p()
        self.params = B.XYZParams((C.c_double * 16)(*q.reshape(16)), int(mode), int(bool(handleMissingValues)),
                                  int(min_disparity), float(max_z))
        self.width, self.height, self.max_batch, self.device = width, height, max_batch, device
        B.check(B.lib().rtdm_xyz_create(C.byref(self.params), width, height, max_batch, device, C.byref(self._h)), "rtdm_xyz_create")

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            try:
                B.lib().rtdm_xyz_destroy(self._h)
            except (TypeError, AttributeError):
                pass
            self._h = None

    __del__ = close

    def set_params(self, **kw):
        """Any of Q, disparity_mode, handle_missing_values, min_disparity, max_z; applies from the next call."""
        p = B.XYZParams()
        C.memmove(C.byref(p), C.byref(self.params), C.sizeof(B.XYZParams))
        for k, v in kw.items():
            if k == "Q":
                q = np.asarray(v, np.float64)
                if q.size != 16:
                    raise ValueError("Q must have 16 entries (4 x 4); got shape %s" % (q.shape,))
                p.Q = (C.c_double * 16)(*q.reshape(16))
            elif k in ("disparity_mode", "handle_missing_values", "min_disparity", "max_z"):
                setattr(p, k, v)
            else:
                raise ValueError("unknown parameter %r" % k)
        B.check(B.lib().rtdm_xyz_set_params(self._h, C.byref(p)), "rtdm_xyz_set_params")
        self.params = p

    @staticmethod
    def _disp(disp):
        d = _wls_plane(disp, np.int16, "disp")
        if d.ndim != 2:
            raise ValueError("disp must be H x W; got shape %s" % (d.shape,))
        return d

    def _map(self, disp, want_xyz, want_z):
        d = self._disp(disp)
        H, W = d.shape
        xyz = np.empty((H, W, 3), np.float32) if want_xyz else None
        z = np.empty((H, W), np.float32) if want_z else None
        B.check(B.lib().rtdm_xyz_map(self._h, d.ctypes.data, d.strides[0], W, H, xyz.ctypes.data if want_xyz else None, W * 12,
                                     z.ctypes.data if want_z else None, W * 4), "rtdm_xyz_map")
        return xyz, z

    def reprojectImageTo3D(self, disp):
        """int16 H x W x16 map -> float32 H x W x 3 (the reference's `xyz`)."""
        return self._map(disp, True, False)[0]

    def depth(self, disp):
        """int16 H x W x16 map -> float32 H x W, the Z plane of reprojectImageTo3D."""
        return self._map(disp, False, True)[1]

    @staticmethod
    def _guide_mask(guide, mask, shape):
        cn, g, m = 0, None, None
        if guide is not None:
            g = _wls_plane(guide, np.uint8, "guide", shape)
            cn = 1 if g.ndim == 2 else g.shape[2]
            if g.ndim not in (2, 3) or cn not in (1, 3):
                raise ValueError("guide must be H x W, H x W x 1 or H x W x 3; got shape %s" % (g.shape,))
        if mask is not None:
            m = _wls_plane(mask, np.uint8, "mask", shape)
            if m.ndim != 2:
                raise ValueError("mask must be H x W; got shape %s" % (m.shape,))
        return cn, g, m

    @staticmethod
    def _capacity(capacity, full):
        cap = full if capacity is None else int(capacity)
        if cap < 0:
            raise ValueError("capacity must not be negative; got %d" % cap)
        return cap

    def cloud(self, disp, guide=None, mask=None, capacity=None):
        """-> (points, count): points is a POINT_DTYPE array of the first min(count, capacity) kept pixels in row-major order,
        count the number of kept pixels.  guide: uint8 H x W (gray) or H x W x 3 (R first); mask: uint8 H x W; capacity: W * H
        when None."""
        d = self._disp(disp)
        H, W = d.shape
        cn, g, m = self._guide_mask(guide, mask, (H, W))
        cap = self._capacity(capacity, W * H)
        pts = np.empty(min(cap, W * H), POINT_DTYPE)
        cnt = C.c_int()
        B.check(B.lib().rtdm_xyz_cloud(self._h, d.ctypes.data, d.strides[0], g.ctypes.data if cn else None, g.strides[0] if cn else 0,
                                       cn, m.ctypes.data if m is not None else None, m.strides[0] if m is not None else 0, W, H,
                                       pts.ctypes.data if pts.size else None, pts.size, C.byref(cnt)), "rtdm_xyz_cloud")
        return pts[:min(cnt.value, pts.size)], cnt.value

    def compute(self, matcher, left, right, guide=None, mask=None, capacity=None, want_disp=False):
        """estimator.cpp:56 + 75-77 in one call (rtdm_bm_compute_cloud): gray pair in, (points, count) out and, with want_disp,
        the matcher's x16 map as well; the map itself stays on the device."""
        if not isinstance(matcher, HIPMatcher):
            raise ValueError("compute runs a StereoBM handle (HIPMatcher); got %s" % type(matcher).__name__)
        l = _wls_plane(left, np.uint8, "left")
        r = _wls_plane(right, np.uint8, "right", l.shape[:2])
        if l.ndim != 2 or r.ndim != 2:
            raise ValueError("compute takes gray frames")
        H, W = l.shape
        cn, g, m = self._guide_mask(guide, mask, (H, W))
        cap = self._capacity(capacity, W * H)
        pts = np.empty(min(cap, W * H), POINT_DTYPE)
        cnt = C.c_int()
        disp = np.empty((H, W), np.int16) if want_disp else None
        B.check(B.lib().rtdm_bm_compute_cloud(matcher._h, self._h, l.ctypes.data, l.strides[0], r.ctypes.data, r.strides[0], W, H,
                                              g.ctypes.data if cn else None, g.strides[0] if cn else 0, cn,
                                              m.ctypes.data if m is not None else None, m.strides[0] if m is not None else 0,
                                              pts.ctypes.data if pts.size else None, pts.size, C.byref(cnt),
                                              disp.ctypes.data if want_disp else None, W * 2), "rtdm_bm_compute_cloud")
        out = (pts[:min(cnt.value, pts.size)], cnt.value)
        return out + (disp,) if want_disp else out

    @staticmethod
    def _dev(t, name, dtype, shape=None):
        """(pointer, row pitch, frame stride) in bytes of an n x H x W [x c] torch tensor whose pixels are contiguous in a row."""
        if t.dtype != dtype:
            raise ValueError("%s must be %s; got %s" % (name, dtype, t.dtype))
        if t.dim() not in (3, 4) or (shape is not None and tuple(t.shape[:3]) != tuple(shape)):
            raise ValueError("%s must be n x H x W%s; got %s" % (name, "" if shape is None else " = %s" % (tuple(shape),), tuple(t.shape)))
        c = t.shape[3] if t.dim() == 4 else 1
        st = t.stride()
        if st[2] != c or (t.dim() == 4 and st[3] != 1) or st[1] < t.shape[2] * c or st[0] < 0:
            raise ValueError("%s rows must be contiguous; got strides %s" % (name, tuple(st)))
        e = t.element_size()
        return t.data_ptr(), st[1] * e, st[0] * e

    def map_device(self, d_disp, d_xyz=None, d_z=None, stream=None):
        """torch device tensors: int16 [n,H,W] in; float32 [n,H,W,3] and / or float32 [n,H,W] out (row pitch and frame stride
        free).  Enqueued on `stream` (a raw hipStream_t value; None = the null stream), not synchronised."""
        import torch
        if d_xyz is None and d_z is None:
            raise ValueError("map_device needs d_xyz, d_z or both")
        dp, dpitch, dframe = self._dev(d_disp, "d_disp", torch.int16)
        n, H, W = d_disp.shape[:3]
        xp = xpitch = xframe = zp = zpitch = zframe = None
        if d_xyz is not None:
            if d_xyz.dim() != 4 or d_xyz.shape[3] != 3:
                raise ValueError("d_xyz must be n x H x W x 3; got %s" % (tuple(d_xyz.shape),))
            xp, xpitch, xframe = self._dev(d_xyz, "d_xyz", torch.float32, (n, H, W))
        if d_z is not None:
            if d_z.dim() != 3:
                raise ValueError("d_z must be n x H x W; got %s" % (tuple(d_z.shape),))
            zp, zpitch, zframe = self._dev(d_z, "d_z", torch.float32, (n, H, W))
        B.check(B.lib().rtdm_xyz_map_device(self._h, n, dp, dpitch, dframe, W, H, xp, xpitch or 0, xframe or 0, zp, zpitch or 0,
                                            zframe or 0, stream), "rtdm_xyz_map_device")

    def cloud_device(self, d_disp, d_points, d_counts, d_guide=None, d_mask=None, capacity=None, stream=None):
        """torch device tensors: int16 [n,H,W] map; d_points: uint8 [n, >= capacity * 16] (frame i's records in row i; view it
        as POINT_DTYPE on the host); d_counts: int32 [n]; optional uint8 guide [n,H,W] or [n,H,W,3] and mask [n,H,W].
        capacity: records per frame, what a row of d_points holds when None.  Enqueued on `stream`, not synchronised."""
        import torch
        dp, dpitch, dframe = self._dev(d_disp, "d_disp", torch.int16)
        n, H, W = d_disp.shape[:3]
        if d_points.dtype != torch.uint8 or d_points.dim() != 2 or d_points.shape[0] != n or d_points.stride(1) != 1:
            raise ValueError("d_points must be uint8 n x bytes; got %s %s" % (d_points.dtype, tuple(d_points.shape)))
        cap = self._capacity(capacity, d_points.shape[1] // 16)
        if cap * 16 > d_points.shape[1]:
            raise ValueError("capacity %d does not fit rows of %d bytes" % (cap, d_points.shape[1]))
        if d_counts.dtype != torch.int32 or d_counts.dim() != 1 or d_counts.shape[0] != n or not d_counts.is_contiguous():
            raise ValueError("d_counts must be a contiguous int32 tensor of n entries")
        cn, gp, gpitch, gframe = 0, None, 0, 0
        if d_guide is not None:
            cn = 1 if d_guide.dim() == 3 else d_guide.shape[3]
            if cn not in (1, 3):
                raise ValueError("d_guide must be n x H x W or n x H x W x 3; got %s" % (tuple(d_guide.shape),))
            gp, gpitch, gframe = self._dev(d_guide, "d_guide", torch.uint8, (n, H, W))
        mp, mpitch, mframe = None, 0, 0
        if d_mask is not None:
            if d_mask.dim() != 3:
                raise ValueError("d_mask must be n x H x W; got %s" % (tuple(d_mask.shape),))
            mp, mpitch, mframe = self._dev(d_mask, "d_mask", torch.uint8, (n, H, W))
        B.check(B.lib().rtdm_xyz_cloud_device(self._h, n, dp, dpitch, dframe, gp, gpitch, gframe, cn, mp, mpitch, mframe, W, H,
                                              d_points.data_ptr(), d_points.stride(0), cap, d_counts.data_ptr(), stream),
                "rtdm_xyz_cloud_device")


MORPH_RECT, MORPH_CROSS, MORPH_ELLIPSE = B.MORPH_RECT, B.MORPH_CROSS, B.MORPH_ELLIPSE
MORPH_ERODE, MORPH_DILATE, MORPH_OPEN, MORPH_CLOSE = B.MORPH_ERODE, B.MORPH_DILATE, B.MORPH_OPEN, B.MORPH_CLOSE
MORPH_GRADIENT, MORPH_TOPHAT, MORPH_BLACKHAT, MORPH_OPEN_CLOSE = B.MORPH_GRADIENT, B.MORPH_TOPHAT, B.MORPH_BLACKHAT, B.MORPH_OPEN_CLOSE


def _make_element(shape, ksize):
    try:
        w, h = (int(v) for v in ksize)
    except (TypeError, ValueError):
        raise ValueError("ksize must be a (width, height) pair; got %r" % (ksize,))
    el = B.MorphElement()
    B.check(B.lib().rtdm_morph_make_element(int(shape), w, h, C.byref(el)), "rtdm_morph_make_element")
    return el


def _element_array(el):
    return np.frombuffer(el.mask, np.uint8, el.width * el.height).reshape(el.height, el.width).astype(bool)


def get_structuring_element(shape, ksize):
    """cv::getStructuringElement(shape, (width, height)) -> bool array height x width (anchor: the centre).  Pure host code."""
    return _element_array(_make_element(shape, ksize))


def _morph_element(element, anchor):
    """element: None (ELLIPSE 10x10), a (shape, (w, h)) pair or a 2-D array (nonzero = member); anchor: (x, y) or None (centre)."""
    if element is None:
        element = (MORPH_ELLIPSE, (10, 10))
    if isinstance(element, (tuple, list)) and len(element) == 2 and np.ndim(element[0]) == 0 and np.ndim(element[1]) == 1:
        el = _make_element(*element)
    else:
        m = np.asarray(element)
        if m.ndim != 2 or m.size == 0:
            raise ValueError("element must be a (shape, (w, h)) pair or a non-empty 2-D array")
        h, w = m.shape
        if w > B.MORPH_MAX_SIZE or h > B.MORPH_MAX_SIZE:
            raise B.RtdmError(-6, "structuring element", "sides above %d are not served" % B.MORPH_MAX_SIZE)
        el = B.MorphElement(w, h, w // 2, h // 2)
        flat = np.ascontiguousarray(m != 0, np.uint8).reshape(-1)
        C.memmove(el.mask, flat.ctypes.data, flat.size)
    if anchor is not None:
        try:
            el.anchor_x, el.anchor_y = (int(v) for v in anchor)
        except (TypeError, ValueError):
            raise ValueError("anchor must be an (x, y) pair; got %r" % (anchor,))
    return el


def _get_morph(fn, handle, where):
    op, it, el = C.c_int(), C.c_int(), B.MorphElement()
    B.check(fn(handle, C.byref(op), C.byref(it), C.byref(el)), where)
    return op.value, _element_array(el), it.value, (el.anchor_x, el.anchor_y)


class HIPMorphologicalFilter:
    """VideoFilterDevice (filter/filter.h:13-37) over rtdm_morph_*; ctor shape of mf-sw.cpp:10-17.  A new filter runs the
    reference's open + close with the 10x10 ellipse; set_op chooses any of cv::morphologyEx's operations, element and
    iteration count (rules M1-M7)."""

    def __init__(self, w, h, bpp=8, max_batch=1, device=0):
        if bpp != 8:
            raise ValueError("only 8 bpp masks are filtered (mf-sw.cpp is called with bpp=8, main.cpp:133)")
        self._h = C.c_void_p()
        self.img_width, self.img_height, self.img_bpp = w, h, bpp
        B.check(B.lib().rtdm_morph_create(w, h, max_batch, device, C.byref(self._h)), "rtdm_morph_create")

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            try:
                B.lib().rtdm_morph_destroy(self._h)
            except (TypeError, AttributeError):
                pass
            self._h = None

    __del__ = close

    def getFrameSize(self):
        return self.img_width * self.img_height * (self.img_bpp >> 3)

    def _buf(self, ptr):
        arr = (C.c_uint8 * self.getFrameSize()).from_address(ptr)
        return np.frombuffer(arr, np.uint8).reshape(self.img_height, self.img_width)

    def getVideoInBuffer(self):
        return self._buf(B.lib().rtdm_morph_in_buffer(self._h))

    def getVideoOutBuffer(self):
        return self._buf(B.lib().rtdm_morph_out_buffer(self._h))

    def set_op(self, op, element=None, iterations=1, anchor=None):
        """From the next run on: op = MORPH_ERODE .. MORPH_BLACKHAT or MORPH_OPEN_CLOSE; element = a (shape, (w, h)) pair, a
        2-D array (nonzero = member) or None for ELLIPSE 10x10; anchor = (x, y), None = (w // 2, h // 2)."""
        el = _morph_element(element, anchor)
        B.check(B.lib().rtdm_morph_set_op(self._h, int(op), int(iterations), C.byref(el)), "rtdm_morph_set_op")

    def get_op(self):
        """-> (op, element as a bool array, iterations, anchor (x, y))"""
        return _get_morph(B.lib().rtdm_morph_get_op, self._h, "rtdm_morph_get_op")

    def run(self, inp, out=None):
        assert inp.dtype == np.uint8 and inp.ndim == 2 and inp.strides[1] == 1
        H, W = inp.shape
        if out is None:
            out = np.empty((H, W), np.uint8)
        B.check(B.lib().rtdm_morph_run(self._h, inp.ctypes.data, inp.strides[0], out.ctypes.data, out.strides[0],
                                       W, H), "rtdm_morph_run")
        return out

    def run_device(self, d_in, d_out, stream=None):
        n, H, W = d_in.shape
        B.check(B.lib().rtdm_morph_run_device(self._h, n, d_in.data_ptr(), W, W * H, d_out.data_ptr(), W, W * H,
                                              W, H, stream), "rtdm_morph_run_device")


class Calibration:
    """What load_calibration read: M1 D1 M2 D2 R T as float64 arrays (D zero-padded to 14), width / height (0 where the
    files have none), and `stored`: the optional keys the files held (ROI1 ROI2 as (x, y, w, h); R1 R2 P1 P2 Q as arrays)."""

    def __init__(self, c, stored):
        self._c, self.stored = c, stored
        self.M1, self.M2, self.R = (np.array(getattr(c, k), np.float64).reshape(3, 3) for k in ("M1", "M2", "R"))
        self.D1, self.D2, self.T = (np.array(getattr(c, k), np.float64) for k in ("D1", "D2", "T"))
        self.width, self.height = c.width, c.height


def _region(r):
    return (r.x, r.y, r.width, r.height)


def _rectification(r):
    out = {k: np.array(getattr(r, k), np.float64).reshape(shape) for k, shape in (("R1", (3, 3)), ("R2", (3, 3)), ("P1", (3, 4)),
                                                                                  ("P2", (3, 4)), ("Q", (4, 4)))}
    out["ROI1"], out["ROI2"] = _region(r.roi1), _region(r.roi2)
    out["_c"] = r
    return out


def load_calibration(intrinsics, extrinsics):
    """main.cpp:61-78: the reference's intrinsics.yml / extrinsics.yml -> Calibration.  Pure host code."""
    c, r, mask = B.Calib(), B.Rectification(), C.c_uint(0)
    B.check(B.lib().rtdm_calib_load(str(intrinsics).encode(), str(extrinsics).encode(), C.byref(c), C.byref(r), C.byref(mask)),
            "rtdm_calib_load")
    full = _rectification(r)
    return Calibration(c, {k: full[k] for k, bit in B.CALIB_HAS.items() if mask.value & bit and k in full})


def stereo_rectify(calib, alpha=-1.0, zero_disparity=True):
    """cv::stereoRectify(M1, D1, M2, D2, size, R, T, ..., flags, alpha, size) -> dict R1 R2 P1 P2 Q ROI1 ROI2 (rules C1-C9,
    DESIGN.md section 4.13).  The defaults are the reference's call (main.cpp:92).  Pure host code."""
    r = B.Rectification()
    B.check(B.lib().rtdm_stereo_rectify(C.byref(calib._c), B.CALIB_ZERO_DISPARITY if zero_disparity else 0, float(alpha), 0, 0,
                                        C.byref(r)), "rtdm_stereo_rectify")
    return _rectification(r)


def init_undistort_rectify_map(M, D, R, P, width, height, device=0):
    """initUndistortRectifyMap(M, D, R, P, (width, height), CV_16SC2) on the device -> (map1 HxWx2 int16, map2 HxW uint16)."""
    m = np.ascontiguousarray(M, np.float64).reshape(9)
    r = np.ascontiguousarray(R, np.float64).reshape(9)
    p = np.ascontiguousarray(P, np.float64).reshape(12)
    dd = np.asarray(D, np.float64).reshape(-1)
    assert dd.size <= 14
    d = np.zeros(14, np.float64)
    d[:dd.size] = dd
    ok = 0 < width <= 32767 and 0 < height <= 32767          # otherwise the call refuses the size and writes nothing
    map1 = np.empty((height, width, 2) if ok else (0, 0, 2), np.int16)
    map2 = np.empty((height, width) if ok else (0, 0), np.uint16)
    B.check(B.lib().rtdm_undistort_rectify_map(m.ctypes.data, d.ctypes.data, r.ctypes.data, p.ctypes.data, width, height, device,
                                               map1.ctypes.data, map2.ctypes.data), "rtdm_undistort_rectify_map")
    return map1, map2


class HIPRectifier:
    """estimator.cpp:29-39 on the device: RGB -> gray -> remap(INTER_LINEAR, CV_16SC2 maps) -> crop to roif.

    map1_*: HxWx2 int16, map2_*: HxW uint16 (what initUndistortRectifyMap(..., CV_16SC2, ...) returns, main.cpp:95-96);
    roi = (x, y, w, h) = the reference's roif (main.cpp:80-85)."""

    def __init__(self, map1_left, map2_left, map1_right, map2_right, roi, max_batch=1, device=0):
        maps = [np.ascontiguousarray(map1_left, np.int16), np.ascontiguousarray(map2_left, np.uint16),
                np.ascontiguousarray(map1_right, np.int16), np.ascontiguousarray(map2_right, np.uint16)]
        H, W = maps[1].shape
        assert maps[0].shape == (H, W, 2) and maps[2].shape == (H, W, 2) and maps[3].shape == (H, W)
        self.width, self.height, self.roi = W, H, tuple(int(v) for v in roi)
        self._h = C.c_void_p()
        B.check(B.lib().rtdm_rectify_create(maps[0].ctypes.data, maps[1].ctypes.data, maps[2].ctypes.data, maps[3].ctypes.data,
                                            W, H, *self.roi, max_batch, device, C.byref(self._h)), "rtdm_rectify_create")

    @classmethod
    def from_calibration(cls, intrinsics, extrinsics, alpha=-1.0, roi="file", max_batch=1, device=0):
        """get_rectified_remap_matrices (main.cpp:53-98) from the two calibration files: stereoRectify with
        CALIB_ZERO_DISPARITY and `alpha`, both cameras' maps built on the device.  roi: "file" = the reference's roif from the
        files' ROI1 / ROI2 (max of the origins, min of the sizes, main.cpp:80-85), "rectify" = the same rule on the computed
        ROIs, or (x, y, w, h).  .Q is stereoRectify's Q (what HIPReprojector and compute_depth take), .rectification the
        whole result, .calibration what the files held."""
        cal = load_calibration(intrinsics, extrinsics)
        rect = stereo_rectify(cal, alpha=alpha, zero_disparity=True)
        if roi == "file":
            if "ROI1" not in cal.stored or "ROI2" not in cal.stored:
                raise ValueError("the calibration files hold no ROI1 / ROI2: pass roi='rectify' or a rectangle")
            r1, r2 = cal.stored["ROI1"], cal.stored["ROI2"]
        elif roi == "rectify":
            r1, r2 = rect["ROI1"], rect["ROI2"]
        else:
            r1 = r2 = tuple(int(v) for v in roi)
        self = cls.__new__(cls)
        self.width, self.height = cal.width, cal.height
        self.roi = (max(r1[0], r2[0]), max(r1[1], r2[1]), min(r1[2], r2[2]), min(r1[3], r2[3]))
        self.calibration, self.rectification, self.Q = cal, rect, rect["Q"]
        self._h = C.c_void_p()
        B.check(B.lib().rtdm_rectify_create_calib(C.byref(cal._c), C.byref(rect["_c"]), *self.roi, max_batch, device,
                                                  C.byref(self._h)), "rtdm_rectify_create_calib")
        return self

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            try:
                B.lib().rtdm_rectify_destroy(self._h)
            except (TypeError, AttributeError):
                pass
            self._h = None

    __del__ = close

    def _check_rgb(self, a):
        assert a.dtype == np.uint8 and a.shape == (self.height, self.width, 3) and a.strides[1] == 3 and a.strides[2] == 1

    def gray(self, rgb_left, rgb_right):
        """-> (left_rect, right_rect), uint8 roi_h x roi_w each."""
        self._check_rgb(rgb_left); self._check_rgb(rgb_right)
        rw, rh = self.roi[2], self.roi[3]
        l = np.empty((rh, rw), np.uint8); r = np.empty((rh, rw), np.uint8)
        B.check(B.lib().rtdm_rectify_gray(self._h, rgb_left.ctypes.data, rgb_left.strides[0], rgb_right.ctypes.data,
                                          rgb_right.strides[0], l.ctypes.data, rw, r.ctypes.data, rw), "rtdm_rectify_gray")
        return l, r

    def rgb(self, rgb, which=0):
        """remap + crop of the colour frame with the left (0) or right (1) maps -> roi_h x roi_w x 3."""
        self._check_rgb(rgb)
        rw, rh = self.roi[2], self.roi[3]
        out = np.empty((rh, rw, 3), np.uint8)
        B.check(B.lib().rtdm_rectify_rgb(self._h, which, rgb.ctypes.data, rgb.strides[0], out.ctypes.data, rw * 3), "rtdm_rectify_rgb")
        return out

    def gray_device(self, d_rgb_left, d_rgb_right, d_left, d_right, stream=None):
        """torch uint8 tensors: [n,H,W,3] x2 -> [n,roi_h,roi_w] x2 (contiguous); ordered on `stream` (None = null stream)."""
        n = d_rgb_left.shape[0]
        B.check(B.lib().rtdm_rectify_gray_device(self._h, n, d_rgb_left.data_ptr(), d_rgb_right.data_ptr(), d_left.data_ptr(),
                                                 d_right.data_ptr(), stream), "rtdm_rectify_gray_device")

    def compute(self, matcher, rgb_left, rgb_right):
        """estimator.cpp:29-36 + 56: raw RGB frames -> x16 disparity of the rectified, cropped pair (host to host)."""
        self._check_rgb(rgb_left); self._check_rgb(rgb_right)
        rw, rh = self.roi[2], self.roi[3]
        disp = np.empty((rh, rw), np.int16)
        B.check(B.lib().rtdm_bm_compute_rgb(matcher._h, self._h, rgb_left.ctypes.data, rgb_left.strides[0], rgb_right.ctypes.data,
                                            rgb_right.strides[0], disp.ctypes.data, rw * 2), "rtdm_bm_compute_rgb")
        return disp

    def compute_device(self, matcher, d_rgb_left, d_rgb_right, d_disp, stream=None):
        n = d_rgb_left.shape[0]
        B.check(B.lib().rtdm_bm_compute_rgb_device(matcher._h, self._h, n, d_rgb_left.data_ptr(), d_rgb_right.data_ptr(),
                                                   d_disp.data_ptr(), stream), "rtdm_bm_compute_rgb_device")


def mjpeg_probe(stream):
    """Headers of one baseline JPEG frame -> dict (width, height, components, h_samp, v_samp, restart_interval, segments,
    has_dht).  Pure host code; raises RtdmError with the status rtdm_mjpeg_probe refuses the frame with."""
    buf = bytes(stream)
    info = B.MJPEGInfo()
    B.check(B.lib().rtdm_mjpeg_probe(buf, len(buf), C.byref(info)), "rtdm_mjpeg_probe")
    return {n: getattr(info, n) for n, _ in B.MJPEGInfo._fields_}


class HIPMJPEGDecoder:
    """The reference's DecoderDevice (include/decoder/decoder.h, estimator.cpp:24-27) on the device: baseline MJPEG frames ->
    interleaved RGB, byte for byte what libjpeg gives with its defaults (JDCT_ISLOW, fancy upsampling).

    width x height: the largest frame; max_stream_bytes: the longest stream (SOI .. EOI).  split: the bytes per subsequence a
    frame without restart intervals is cut into, one lane each (rtdm_mjpeg_set_split): None or -1 = the built-in default,
    0 = off, 8 .. 65536."""

    def __init__(self, width, height, max_batch=1, max_stream_bytes=None, device=0, split=None):
        self.width, self.height, self.max_batch, self.device = int(width), int(height), int(max_batch), device
        self.max_stream_bytes = int(max_stream_bytes) if max_stream_bytes else max(4096, self.width * self.height * 3)
        self._h = C.c_void_p()
        B.check(B.lib().rtdm_mjpeg_create(self.width, self.height, self.max_batch, self.max_stream_bytes, device,
                                          C.byref(self._h)), "rtdm_mjpeg_create")
        if split is not None:
            self.split = split

    @property
    def split(self):
        v = C.c_int()
        B.check(B.lib().rtdm_mjpeg_get_split(self._h, C.byref(v)), "rtdm_mjpeg_get_split")
        return v.value

    @split.setter
    def split(self, subsequence_bytes):
        B.check(B.lib().rtdm_mjpeg_set_split(self._h, -1 if subsequence_bytes is None else int(subsequence_bytes)),
                "rtdm_mjpeg_set_split")

    def split_stats(self):
        """(frames decoded the split way, their subsequences, the most rounds one took) since creation.  Synchronises the stream
        of the last call."""
        f, n, r = C.c_long(), C.c_long(), C.c_int()
        B.check(B.lib().rtdm_mjpeg_get_split_stats(self._h, C.byref(f), C.byref(n), C.byref(r)), "rtdm_mjpeg_get_split_stats")
        return f.value, n.value, r.value

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            try:
                B.lib().rtdm_mjpeg_destroy(self._h)
            except (TypeError, AttributeError):
                pass
            self._h = None

    __del__ = close

    def decode(self, stream, out=None):
        """bytes -> H x W x 3 uint8 (host to host, synchronous); the size comes from the frame's own header."""
        buf = bytes(stream)
        info = mjpeg_probe(buf)
        W, H = info["width"], info["height"]
        if out is None:
            out = np.empty((H, W, 3), np.uint8)
        assert out.dtype == np.uint8 and out.shape == (H, W, 3) and out.strides[1] == 3 and out.strides[2] == 1
        B.check(B.lib().rtdm_mjpeg_decode(self._h, buf, len(buf), W, H, out.ctypes.data, out.strides[0]), "rtdm_mjpeg_decode")
        return out

    def decode_batch(self, streams, out=None, status=None, stream=None):
        """list of bytes (frames of one size and sampling) -> torch uint8 [n, H, W, 3] on the device, enqueued on `stream`
        (None = the null stream) and not synchronised.  out: a tensor to fill; its strides give pitch and frame stride.
        status (optional): torch int32 [n], 0 or -8 (damaged entropy data) per frame."""
        import torch
        bufs = [bytes(s) for s in streams]
        n = len(bufs)
        info = mjpeg_probe(bufs[0])
        W, H = info["width"], info["height"]
        if out is None:
            out = torch.empty((n, H, W, 3), dtype=torch.uint8, device="cuda:%d" % self.device)
        assert out.dtype == torch.uint8 and tuple(out.shape) == (n, H, W, 3) and out.stride(3) == 1 and out.stride(2) == 3
        if status is not None:
            assert status.dtype == torch.int32 and status.numel() == n and status.is_contiguous()
        ptrs = (C.c_void_p * n)(*[C.cast(C.c_char_p(b), C.c_void_p) for b in bufs])
        lens = (C.c_size_t * n)(*[len(b) for b in bufs])
        B.check(B.lib().rtdm_mjpeg_decode_batch_device(self._h, n, ptrs, lens, W, H, out.data_ptr(), out.stride(1), out.stride(0),
                                                       status.data_ptr() if status is not None else None, stream),
                "rtdm_mjpeg_decode_batch_device")
        return out

    def compute(self, matcher, rectifier, left, right):
        """estimator.cpp:24-36 + 56: the two cameras' MJPEG frames -> x16 disparity of the rectified, cropped pair."""
        l, r = bytes(left), bytes(right)
        rw, rh = rectifier.roi[2], rectifier.roi[3]
        disp = np.empty((rh, rw), np.int16)
        B.check(B.lib().rtdm_bm_compute_mjpeg(matcher._h, rectifier._h, self._h, l, len(l), r, len(r), rectifier.width,
                                              rectifier.height, disp.ctypes.data, rw * 2), "rtdm_bm_compute_mjpeg")
        return disp


HSV_LOW, HSV_HIGH = (0, 150, 0), (9, 255, 255)          # the reference's red filter, estimator.cpp:110-115


def _hsv_range(low, high):
    return B.HsvRange((C.c_int * 3)(*[int(v) for v in low]), (C.c_int * 3)(*[int(v) for v in high]))


OBJECT_DTYPE = np.dtype([(n, "<i4") for n in ("x", "y", "width", "height", "cls", "first_pixel")] + [("reserved", "<i4", (2,))])   # rtdm_object


def _hsv_classes(ranges, classes):
    """ranges: [(low, high)], classes: one class id per range (None: one class per range) -> (HsvRange[], int[], nranges, nclasses)."""
    ranges = list(ranges)
    classes = list(range(len(ranges))) if classes is None else [int(c) for c in classes]
    if len(classes) != len(ranges):
        raise ValueError("%d ranges but %d class ids" % (len(ranges), len(classes)))
    n = len(ranges)
    rng = (B.HsvRange * max(n, 1))(*[_hsv_range(lo, hi) for lo, hi in ranges])
    cls = (C.c_int * max(n, 1))(*classes)
    return rng, cls, n, (max(classes) + 1 if classes else 0)


class HIPObjectDetector:
    """estimator.cpp:40-53 on the device: HSV threshold -> morphological filter -> external components -> boxes.  The filter
    is the reference's open + close with the 10x10 ellipse unless set_op chose another (as HIPMorphologicalFilter.set_op).
    max_batch frames x max_classes colour classes go through one launch of the batched calls (detect_classes, detect_device)."""

    def __init__(self, width, height, device=0, max_batch=1, max_classes=1):
        self.width, self.height, self.max_batch, self.max_classes = width, height, max_batch, max_classes
        self._h = C.c_void_p()
        B.check(B.lib().rtdm_objects_create_batch(width, height, max_batch, max_classes, device, C.byref(self._h)),
                "rtdm_objects_create_batch")

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            try:
                B.lib().rtdm_objects_destroy(self._h)
            except (TypeError, AttributeError):
                pass
            self._h = None

    __del__ = close

    def set_op(self, op, element=None, iterations=1, anchor=None):
        el = _morph_element(element, anchor)
        B.check(B.lib().rtdm_objects_set_morph(self._h, int(op), int(iterations), C.byref(el)), "rtdm_objects_set_morph")

    def get_op(self):
        return _get_morph(B.lib().rtdm_objects_get_morph, self._h, "rtdm_objects_get_morph")

    def detect(self, rgb, low=HSV_LOW, high=HSV_HIGH, min_area=100, zero_border=True, max_boxes=256):
        """rgb: HxWx3 uint8 (R first) -> (boxes [(x,y,w,h)], roi (x,y,w,h), mask HxW uint8 = filter_out)."""
        assert rgb.dtype == np.uint8 and rgb.shape == (self.height, self.width, 3) and rgb.strides[1] == 3 and rgb.strides[2] == 1
        boxes = (B.Region * max_boxes)(); n = C.c_int(); roi = B.Region()
        mask = np.empty((self.height, self.width), np.uint8)
        rng = _hsv_range(low, high)
        B.check(B.lib().rtdm_objects_detect(self._h, rgb.ctypes.data, rgb.strides[0], C.byref(rng), min_area, int(zero_border),
                                            mask.ctypes.data, self.width, boxes, max_boxes, C.byref(n), C.byref(roi)),
                "rtdm_objects_detect")
        out = [(b.x, b.y, b.width, b.height) for b in boxes[:min(n.value, max_boxes)]]
        return out, (roi.x, roi.y, roi.width, roi.height), mask

    def detect_classes(self, rgbs, ranges, classes=None, min_area=100, zero_border=True, capacity=256, want_masks=True):
        """rgbs: n x H x W x 3 uint8 (R first); ranges: [(low, high)]; classes: the class id of every range (None: one class
        per range) -> (objects, rois, counts, masks): per frame the list of (x, y, w, h, cls) -- class ascending, at most
        `capacity` of them --, the union box (x, y, w, h) of all of the frame's objects, counts n x nclasses (not clipped) and
        the filtered masks n x nclasses x H x W (None without want_masks)."""
        rgbs = np.asarray(rgbs)
        if rgbs.dtype != np.uint8 or rgbs.ndim != 4 or rgbs.shape[1:] != (self.height, self.width, 3):
            raise ValueError("rgbs must be uint8 n x %d x %d x 3; got %s %s" % (self.height, self.width, rgbs.dtype, rgbs.shape))
        if rgbs.strides[2] != 3 or rgbs.strides[3] != 1 or rgbs.strides[1] < 3 * self.width or rgbs.strides[0] < 0:
            raise ValueError("the pixels of a row must be contiguous; got strides %s" % (rgbs.strides,))
        rng, cls, nr, K = _hsv_classes(ranges, classes)
        n, H, W = rgbs.shape[0], self.height, self.width
        objs = np.zeros((n, capacity), OBJECT_DTYPE)
        counts = np.zeros((n, max(K, 1)), np.int32); rois = np.zeros((n, 4), np.int32)
        masks = np.empty((n, max(K, 1), H, W), np.uint8) if want_masks else None
        B.check(B.lib().rtdm_objects_detect_batch(self._h, n, rgbs.ctypes.data, rgbs.strides[1], rgbs.strides[0], rng, cls, nr, K,
                                                  int(min_area), int(zero_border), masks.ctypes.data if want_masks else None, W, W * H,
                                                  objs.ctypes.data, capacity, counts.ctypes.data, rois.ctypes.data),
                "rtdm_objects_detect_batch")
        out = []
        for f in range(n):
            o = objs[f, :min(int(counts[f].sum()), capacity)]
            out.append(list(zip(o["x"].tolist(), o["y"].tolist(), o["width"].tolist(), o["height"].tolist(), o["cls"].tolist())))
        return out, [tuple(int(v) for v in r) for r in rois], counts, masks

    def detect_device(self, d_rgb, ranges, classes, d_objects, d_counts, d_rois, d_masks=None, min_area=100, zero_border=True,
                      capacity=None, stream=None):
        """torch device tensors: uint8 [n,H,W,3] frames (row pitch and frame stride free); d_objects: uint8 [n, >= capacity * 32]
        (frame i's records in row i, rows contiguous; view it as OBJECT_DTYPE on the host); d_counts: int32 [n, nclasses];
        d_rois: int32 [n, 4]; optional d_masks: uint8 [n, nclasses, H, W] (row pitch and plane stride free).  capacity: records
        per frame, what a row of d_objects holds when None.  Enqueued on `stream` (a raw hipStream_t value; None = the null
        stream), not synchronised."""
        import torch
        rng, cls, nr, K = _hsv_classes(ranges, classes)
        if d_rgb.dtype != torch.uint8 or d_rgb.dim() != 4 or tuple(d_rgb.shape[1:]) != (self.height, self.width, 3):
            raise ValueError("d_rgb must be uint8 n x %d x %d x 3; got %s %s" % (self.height, self.width, d_rgb.dtype, tuple(d_rgb.shape)))
        rp, rpitch, rframe = HIPReprojector._dev(d_rgb, "d_rgb", torch.uint8)
        n, H, W = d_rgb.shape[0], self.height, self.width
        if d_objects.dtype != torch.uint8 or d_objects.dim() != 2 or d_objects.shape[0] != n or not d_objects.is_contiguous():
            raise ValueError("d_objects must be a contiguous uint8 tensor of n rows; got %s %s" % (d_objects.dtype, tuple(d_objects.shape)))
        if capacity is None:
            capacity = d_objects.shape[1] // 32
        if capacity < 0 or capacity * 32 != d_objects.shape[1]:
            raise ValueError("rows of d_objects must hold exactly capacity * 32 bytes; got %d for capacity %d" % (d_objects.shape[1], capacity))
        if d_counts.dtype != torch.int32 or tuple(d_counts.shape) != (n, K) or not d_counts.is_contiguous():
            raise ValueError("d_counts must be a contiguous int32 tensor n x nclasses")
        if d_rois.dtype != torch.int32 or tuple(d_rois.shape) != (n, 4) or not d_rois.is_contiguous():
            raise ValueError("d_rois must be a contiguous int32 tensor n x 4")
        mp, mpitch, mplane = None, 0, 0
        if d_masks is not None:
            if d_masks.dtype != torch.uint8 or tuple(d_masks.shape) != (n, K, H, W):
                raise ValueError("d_masks must be uint8 n x nclasses x H x W; got %s %s" % (d_masks.dtype, tuple(d_masks.shape)))
            st = d_masks.stride()
            if st[3] != 1 or st[2] < W or st[1] < st[2] * H or (n > 1 and st[0] != K * st[1]):
                raise ValueError("d_masks: contiguous rows and one stride from plane to plane; got strides %s" % (tuple(st),))
            mp, mpitch, mplane = d_masks.data_ptr(), st[2], st[1]
        B.check(B.lib().rtdm_objects_detect_device(self._h, n, rp, rpitch, rframe, rng, cls, nr, K, int(min_area), int(zero_border),
                                                   mp, mpitch, mplane, d_objects.data_ptr(), capacity, d_counts.data_ptr(),
                                                   d_rois.data_ptr(), stream), "rtdm_objects_detect_device")


def estimate_frame(matcher, rectifier, detector, rgb_left, rgb_right, Q, low=HSV_LOW, high=HSV_HIGH, min_area=100,
                   zero_border=True, calibration_unit=25.0, max_boxes=64, want_disp=False):
    """One iteration of Estimator::run (estimator.cpp:29-77) without capture/decode/drawing:
    -> (boxes, mean_cm, counts[, disp])."""
    rectifier._check_rgb(rgb_left); rectifier._check_rgb(rgb_right)
    rw, rh = rectifier.roi[2], rectifier.roi[3]
    boxes = (B.Region * max_boxes)(); n = C.c_int()
    mean = np.zeros(max_boxes, np.float64); cnt = np.zeros(max_boxes, np.int32)
    q = np.ascontiguousarray(Q, np.float64).reshape(16)
    disp = np.empty((rh, rw), np.int16) if want_disp else None
    rng = _hsv_range(low, high)
    B.check(B.lib().rtdm_estimate_frame(matcher._h, rectifier._h, detector._h, rgb_left.ctypes.data, rgb_left.strides[0],
                                        rgb_right.ctypes.data, rgb_right.strides[0], q.ctypes.data_as(C.POINTER(C.c_double)),
                                        C.byref(rng), min_area, int(zero_border), calibration_unit, boxes,
                                        mean.ctypes.data_as(C.POINTER(C.c_double)), cnt.ctypes.data_as(C.POINTER(C.c_int)),
                                        max_boxes, C.byref(n), disp.ctypes.data if want_disp else None, rw * 2),
            "rtdm_estimate_frame")
    k = min(n.value, max_boxes)
    out = [(b.x, b.y, b.width, b.height) for b in boxes[:k]]
    return (out, mean[:k], cnt[:k], disp) if want_disp else (out, mean[:k], cnt[:k])


def estimate_frame_classes(matcher, rectifier, detector, rgb_left, rgb_right, Q, ranges, classes=None, min_area=100,
                           zero_border=True, calibration_unit=25.0, max_objects=64, want_disp=False):
    """estimate_frame for several colour classes (ranges / classes as HIPObjectDetector.detect_classes): the matcher's ROI is
    the union box over all classes, every object is measured under the mask of its own class
    -> (objects [(x, y, w, h, cls)], mean_cm, counts[, disp])."""
    rectifier._check_rgb(rgb_left); rectifier._check_rgb(rgb_right)
    rw, rh = rectifier.roi[2], rectifier.roi[3]
    objs = np.zeros(max_objects, OBJECT_DTYPE); n = C.c_int()
    mean = np.zeros(max_objects, np.float64); cnt = np.zeros(max_objects, np.int32)
    q = np.ascontiguousarray(Q, np.float64).reshape(16)
    disp = np.empty((rh, rw), np.int16) if want_disp else None
    rng, cls, nr, K = _hsv_classes(ranges, classes)
    B.check(B.lib().rtdm_estimate_frame_classes(matcher._h, rectifier._h, detector._h, rgb_left.ctypes.data, rgb_left.strides[0],
                                                rgb_right.ctypes.data, rgb_right.strides[0], q.ctypes.data_as(C.POINTER(C.c_double)),
                                                rng, cls, nr, K, int(min_area), int(zero_border), calibration_unit, objs.ctypes.data,
                                                mean.ctypes.data_as(C.POINTER(C.c_double)), cnt.ctypes.data_as(C.POINTER(C.c_int)),
                                                max_objects, C.byref(n), disp.ctypes.data if want_disp else None, rw * 2),
            "rtdm_estimate_frame_classes")
    k = min(n.value, max_objects)
    o = objs[:k]
    out = list(zip(o["x"].tolist(), o["y"].tolist(), o["width"].tolist(), o["height"].tolist(), o["cls"].tolist()))
    k = min(k, B.MAX_REGIONS)
    return (out, mean[:k], cnt[:k], disp) if want_disp else (out, mean[:k], cnt[:k])


def depth_stats_device(d_disp, Q, d_mask, regions, calibration_unit=25.0, device=0, stream=None):
    """torch CUDA tensors: int16 [H,W] x16 disparity, uint8 [H,W] mask -> (mean_cm[n], counts[n]); synchronous."""
    H, W = d_disp.shape
    q = np.ascontiguousarray(Q, np.float64).reshape(16)
    n = len(regions)
    reg = (B.Region * max(n, 1))(*[B.Region(*[int(v) for v in r]) for r in regions])
    mean = np.zeros(n, np.float64); cnt = np.zeros(n, np.int32)
    B.check(B.lib().rtdm_depth_stats_device(device, d_disp.data_ptr(), W * 2, W, H, q.ctypes.data_as(C.POINTER(C.c_double)),
                                            d_mask.data_ptr(), W, reg, n, calibration_unit,
                                            mean.ctypes.data_as(C.POINTER(C.c_double)), cnt.ctypes.data_as(C.POINTER(C.c_int)),
                                            stream), "rtdm_depth_stats_device")
    return mean, cnt


def depth_objects_workspace_bytes(n, capacity, height):
    return int(B.lib().rtdm_depth_objects_workspace_bytes(int(n), int(capacity), int(height)))


def depth_objects_device(d_disp, Q, d_masks, d_objects, d_counts, d_mean_cm, d_npix, calibration_unit=25.0, capacity=None,
                         d_workspace=None, device=0, stream=None):
    """The mean depth of every object of n frames from the detector's device lists (rtdm_depth_objects_device, rules D1-D6).
    torch device tensors: d_disp int16 [n,H,W] x16 maps and d_masks uint8 [n,nclasses,H,W] (row pitch and frame / plane stride
    free), d_objects uint8 [n, capacity * 32] and d_counts int32 [n, nclasses] as HIPObjectDetector.detect_device leaves them,
    d_mean_cm float64 [n, capacity] and d_npix int32 [n, capacity] (written for the stored objects only).  d_workspace: a uint8
    tensor of at least depth_objects_workspace_bytes(n, capacity, H) bytes (None: one is allocated through torch and returned;
    keep it until the work has finished).  Enqueued on `stream` (a raw hipStream_t value; None = the null stream), not
    synchronised.  -> the workspace tensor."""
    import torch
    dp, dpitch, dframe = HIPReprojector._dev(d_disp, "d_disp", torch.int16)
    n, H, W = d_disp.shape
    if d_masks.dtype != torch.uint8 or d_masks.dim() != 4 or d_masks.shape[0] != n or tuple(d_masks.shape[2:]) != (H, W):
        raise ValueError("d_masks must be uint8 n x nclasses x H x W; got %s %s" % (d_masks.dtype, tuple(d_masks.shape)))
    K = d_masks.shape[1]
    st = d_masks.stride()
    if st[3] != 1 or st[2] < W or st[1] < st[2] * H or (n > 1 and st[0] != K * st[1]):
        raise ValueError("d_masks: contiguous rows and one stride from plane to plane; got strides %s" % (tuple(st),))
    if d_objects.dtype != torch.uint8 or d_objects.dim() != 2 or d_objects.shape[0] != n or not d_objects.is_contiguous():
        raise ValueError("d_objects must be a contiguous uint8 tensor of n rows; got %s %s" % (d_objects.dtype, tuple(d_objects.shape)))
    if capacity is None:
        capacity = d_objects.shape[1] // 32
    if capacity < 0 or capacity * 32 != d_objects.shape[1]:
        raise ValueError("rows of d_objects must hold exactly capacity * 32 bytes; got %d for capacity %d" % (d_objects.shape[1], capacity))
    if d_counts.dtype != torch.int32 or tuple(d_counts.shape) != (n, K) or not d_counts.is_contiguous():
        raise ValueError("d_counts must be a contiguous int32 tensor n x nclasses")
    if d_mean_cm.dtype != torch.float64 or tuple(d_mean_cm.shape) != (n, capacity) or not d_mean_cm.is_contiguous():
        raise ValueError("d_mean_cm must be a contiguous float64 tensor n x capacity")
    if d_npix.dtype != torch.int32 or tuple(d_npix.shape) != (n, capacity) or not d_npix.is_contiguous():
        raise ValueError("d_npix must be a contiguous int32 tensor n x capacity")
    need = depth_objects_workspace_bytes(n, capacity, H)
    if d_workspace is None:
        d_workspace = torch.empty(need, dtype=torch.uint8, device=d_disp.device)
    q = np.ascontiguousarray(Q, np.float64).reshape(16)
    B.check(B.lib().rtdm_depth_objects_device(device, n, dp, dpitch, dframe, W, H, q.ctypes.data_as(C.POINTER(C.c_double)),
                                              d_masks.data_ptr(), st[2], st[1], K, d_objects.data_ptr(), capacity, d_counts.data_ptr(),
                                              calibration_unit, d_mean_cm.data_ptr(), d_npix.data_ptr(), d_workspace.data_ptr(),
                                              d_workspace.numel(), stream), "rtdm_depth_objects_device")
    return d_workspace


class HIPEstimator:
    """The loop body of Estimator::run (estimator.cpp:29-77) on frame batches: rtdm_estimate_batch.  Borrows a HIPMatcher, a
    HIPRectifier and a HIPObjectDetector (keep them alive; close this first); a chunk is min(max_batch, the matcher's, the
    detector's max_batch) frames, `capacity` objects of a frame are stored and measured."""

    def __init__(self, matcher, rectifier, detector, max_batch=1, capacity=256):
        self.matcher, self.rectifier, self.detector = matcher, rectifier, detector
        self.max_batch, self.capacity = int(max_batch), int(capacity)
        self._h = C.c_void_p()
        B.check(B.lib().rtdm_estimator_create(matcher._h, rectifier._h, detector._h, self.max_batch, self.capacity, C.byref(self._h)),
                "rtdm_estimator_create")

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            try:
                B.lib().rtdm_estimator_destroy(self._h)
            except (TypeError, AttributeError):
                pass
            self._h = None

    __del__ = close

    def estimate(self, rgb_left, rgb_right, Q, ranges, classes=None, min_area=100, zero_border=True, calibration_unit=25.0,
                 want_disp=False, disp=None):
        """rgb_left / rgb_right: n x H x W x 3 uint8 (R first; row pitch and frame stride free) -> (objects, counts, mean_cm,
        npix[, disp]): per frame the list of (x, y, w, h, cls) -- at most `capacity` --, counts n x nclasses (not clipped), and
        per frame the arrays of its stored objects' mean depth [cm] and pixel count.  disp: n x crop H x crop W int16; frames
        without objects keep what it held (zeros when it is allocated here)."""
        rc = self.rectifier
        rgb_left, rgb_right = np.asarray(rgb_left), np.asarray(rgb_right)
        for a in (rgb_left, rgb_right):
            if a.dtype != np.uint8 or a.ndim != 4 or a.shape[1:] != (rc.height, rc.width, 3) or a.shape[0] != rgb_left.shape[0]:
                raise ValueError("frames must be uint8 n x %d x %d x 3; got %s %s" % (rc.height, rc.width, a.dtype, a.shape))
            if a.strides[2] != 3 or a.strides[3] != 1 or a.strides[1] < 3 * rc.width or a.strides[0] < 0:
                raise ValueError("the pixels of a row must be contiguous; got strides %s" % (a.strides,))
        n, cap = rgb_left.shape[0], self.capacity
        rw, rh = rc.roi[2], rc.roi[3]
        rng, cls, nr, K = _hsv_classes(ranges, classes)
        objs = np.zeros((n, cap), OBJECT_DTYPE); counts = np.zeros((n, max(K, 1)), np.int32)
        mean = np.zeros((n, cap), np.float64); npix = np.zeros((n, cap), np.int32)
        if want_disp and disp is None:
            disp = np.zeros((n, rh, rw), np.int16)
        if disp is not None and (disp.dtype != np.int16 or disp.shape != (n, rh, rw) or not disp.flags.c_contiguous):
            raise ValueError("disp must be a contiguous int16 array %s" % ((n, rh, rw),))
        q = np.ascontiguousarray(Q, np.float64).reshape(16)
        B.check(B.lib().rtdm_estimate_batch(self._h, n, rgb_left.ctypes.data, rgb_left.strides[1], rgb_left.strides[0],
                                            rgb_right.ctypes.data, rgb_right.strides[1], rgb_right.strides[0],
                                            q.ctypes.data_as(C.POINTER(C.c_double)), rng, cls, nr, K, int(min_area), int(zero_border),
                                            calibration_unit, objs.ctypes.data, counts.ctypes.data, mean.ctypes.data, npix.ctypes.data,
                                            disp.ctypes.data if disp is not None else None, rw * 2, rw * rh * 2), "rtdm_estimate_batch")
        out, means, pixels = [], [], []
        for f in range(n):
            k = min(int(counts[f].sum()), cap)
            o = objs[f, :k]
            out.append(list(zip(o["x"].tolist(), o["y"].tolist(), o["width"].tolist(), o["height"].tolist(), o["cls"].tolist())))
            means.append(mean[f, :k].copy()); pixels.append(npix[f, :k].copy())
        return (out, counts, means, pixels, disp) if disp is not None else (out, counts, means, pixels)

    def estimate_device(self, d_rgb_left, d_rgb_right, Q, ranges, classes, d_objects, d_counts, d_mean_cm, d_npix, d_disp=None,
                        min_area=100, zero_border=True, calibration_unit=25.0, stream=None):
        """torch device tensors: uint8 [n,H,W,3] frames (row pitch and frame stride free); d_objects uint8 [n, capacity * 32],
        d_counts int32 [n, nclasses], d_mean_cm float64 [n, capacity], d_npix int32 [n, capacity], optional d_disp int16
        [n, crop H, crop W] (row pitch and frame stride free).  Enqueued on `stream` (a raw hipStream_t value; None = the null
        stream), which is synchronised once per chunk; the results are complete on the stream, not synchronised."""
        import torch
        rc, cap = self.rectifier, self.capacity
        rng, cls, nr, K = _hsv_classes(ranges, classes)
        n = d_rgb_left.shape[0]
        ptr = []
        for t, name in ((d_rgb_left, "d_rgb_left"), (d_rgb_right, "d_rgb_right")):
            if t.dim() != 4 or tuple(t.shape) != (n, rc.height, rc.width, 3):
                raise ValueError("%s must be uint8 n x %d x %d x 3; got %s" % (name, rc.height, rc.width, tuple(t.shape)))
            ptr.append(HIPReprojector._dev(t, name, torch.uint8))
        for t, name, dtype, shape in ((d_objects, "d_objects", torch.uint8, (n, cap * 32)), (d_counts, "d_counts", torch.int32, (n, K)),
                                      (d_mean_cm, "d_mean_cm", torch.float64, (n, cap)), (d_npix, "d_npix", torch.int32, (n, cap))):
            if t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous():
                raise ValueError("%s must be a contiguous %s tensor %s; got %s %s" % (name, dtype, shape, t.dtype, tuple(t.shape)))
        dp, dpitch, dframe = None, 0, 0
        if d_disp is not None:
            dp, dpitch, dframe = HIPReprojector._dev(d_disp, "d_disp", torch.int16, (n, rc.roi[3], rc.roi[2]))
        q = np.ascontiguousarray(Q, np.float64).reshape(16)
        (lp, lpitch, lframe), (rp, rpitch, rframe) = ptr
        B.check(B.lib().rtdm_estimate_batch_device(self._h, n, lp, lpitch, lframe, rp, rpitch, rframe, q.ctypes.data_as(C.POINTER(C.c_double)),
                                                   rng, cls, nr, K, int(min_area), int(zero_border), calibration_unit,
                                                   d_objects.data_ptr(), d_counts.data_ptr(), d_mean_cm.data_ptr(), d_npix.data_ptr(),
                                                   dp, dpitch, dframe, stream), "rtdm_estimate_batch_device")


def synth_pairs_device(d_left, d_right, first_frame, numDisparities, seed=None, device=0, stream=None):
    """Fill torch uint8 [n,H,W] tensors with frames [first_frame, first_frame+n) of the stream."""
    from . import synth
    n, H, W = d_left.shape
    B.check(B.lib().rtdm_synth_pairs_device(synth.STREAM_SEED if seed is None else seed, first_frame, n, W, H,
                                            numDisparities, d_left.data_ptr(), d_right.data_ptr(), W, W * H,
                                            device, stream), "rtdm_synth_pairs_device")
