"""The two matchers over rtdm_bm_* and rtdm_sgm_* (csrc/api_bm.hip, csrc/api_sgm.hip)."""
import ctypes as C

import numpy as np

from . import binding as B
from ._marshal import Handle, q16, regions_array

PREFILTER_NORMALIZED_RESPONSE, PREFILTER_XSOBEL = B.PREFILTER_NORMALIZED_RESPONSE, B.PREFILTER_XSOBEL


class HIPMatcher(Handle):
    """numOfDisparities: any multiple of 16 with minDisparity + numOfDisparities <= 2047 (up to 4080), any odd blockSize
    5..255 -- the parameters go to rtdm_bm_create unchanged; only frames wider than 4096 are refused.
    preFilterType (PREFILTER_XSOBEL, PREFILTER_NORMALIZED_RESPONSE) and preFilterSize (odd, 5..255) are cv::StereoBM's;
    they go through rtdm_bm_set_prefilter, at construction and by setPreFilterType / setPreFilterSize."""
    _destroy = "rtdm_bm_destroy"

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
        n = len(regions)
        mean = np.zeros(n, np.float64); cnt = np.zeros(n, np.int32)
        disp = np.empty((H, W), np.int16) if want_disp else None
        B.check(B.lib().rtdm_bm_compute_depth(
            self._h, left.ctypes.data, left.strides[0], right.ctypes.data, right.strides[0], W, H,
            q16(Q), mask.ctypes.data, mask.strides[0], regions_array(regions), n, calibration_unit,
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

    def compute_device(self, d_left, d_right, d_disp, stream=None, rois=None):
        """torch CUDA tensors: uint8 [n,H,W] x2, int16 [n,H,W]; enqueued on ``stream`` (a raw
        hipStream_t value, e.g. torch.cuda.current_stream().cuda_stream), not synchronised.
        rois: a contiguous int32 [n, 4] device tensor (x, y, w, h) -- frame f runs under ROI1 = rois[f], read on the device
        (rtdm_bm_compute_device_rois); a frame with w <= 0 or h <= 0 is skipped, its plane keeps what it held."""
        n, H, W = d_left.shape
        assert d_left.is_contiguous() and d_right.is_contiguous() and d_disp.is_contiguous()
        if rois is None:
            B.check(B.lib().rtdm_bm_compute_device(self._h, n, d_left.data_ptr(), d_right.data_ptr(), W, W * H, W, H,
                                                   d_disp.data_ptr(), W * 2, W * H * 2, stream), "rtdm_bm_compute_device")
            return
        import torch
        if not isinstance(rois, torch.Tensor) or rois.dtype != torch.int32 or tuple(rois.shape) != (n, 4) or not rois.is_contiguous() \
                or rois.device != d_left.device:
            raise ValueError("rois must be a contiguous int32 tensor (%d, 4) on %s; got %s" % (
                n, d_left.device, "%s %s on %s" % (rois.dtype, tuple(rois.shape), rois.device) if isinstance(rois, torch.Tensor)
                else type(rois).__name__))
        B.check(B.lib().rtdm_bm_compute_device_rois(self._h, n, d_left.data_ptr(), d_right.data_ptr(), W, W * H, W, H, rois.data_ptr(),
                                                    d_disp.data_ptr(), W * 2, W * H * 2, stream), "rtdm_bm_compute_device_rois")

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


class HIPSemiGlobalMatcher(Handle):
    """BlockMatcher over rtdm_sgm_*; constructor shape of SWSemiGlobalMatcher
    (include/stereo-matcher/sgbm-sw.h:27-28): blockSize, minDisparity, numOfDisparities, uniquenessRatio,
    speckleWindowSize, speckleRange, disp12MaxDiff; P1/P2 are the literals of sgbm-sw.cpp:17-18.  numOfDisparities is
    any multiple of 16, as in cv::StereoSGBM (above 256 the path passes run on the wide-line kernel); the library checks it.
    preFilterCap is cv::StereoSGBM's (0 .. 127, setPreFilterCap); compute / compute_device take gray (H x W) or
    interleaved colour (H x W x 3) uint8 frames, as cv::StereoSGBM::compute takes CV_8UC1 and CV_8UC3.
    mode is cv::StereoSGBM::setMode's value (MODE_SGBM, MODE_HH, MODE_HH4; MODE_SGBM_3WAY is refused at creation with
    RTDM_ERR_UNSUPPORTED and served by setMode on the live matcher); paths names the same thing by its direction count (5, 8, 4)
    and defaults to 8.
    cost is the pixel cost: COST_BT (the default, cv::StereoSGBM's) or COST_CENSUS, the Hamming distance of census descriptors
    over a census = (width, height) window, width in 3, 5, 7, 9 and height in 3, 5, 7 -- this project's own, with no library
    counterpart, for pairs whose cameras expose differently (gray frames only; rtdm_sgm_set_cost in include/rtdm.h)."""
    _destroy = "rtdm_sgm_destroy"
    COST_BT, COST_CENSUS = B.SGM_COST_BT, B.SGM_COST_CENSUS
    _CENSUS_W, _CENSUS_H = (3, 5, 7, 9), (3, 5, 7)

    MODE_SGBM, MODE_HH, MODE_SGBM_3WAY, MODE_HH4 = 0, 1, 2, 3          # cv::StereoSGBM's values
    _MODE_PATHS = {MODE_SGBM: 5, MODE_HH: 8, MODE_SGBM_3WAY: 3, MODE_HH4: 4}

    def __init__(self, blockSize=5, minDisparity=0, numOfDisparities=128, uniquenessRatio=10, speckleWindowSize=100,
                 speckleRange=32, disp12MaxDiff=1, P1=600, P2=2400, width=1280, height=720, max_batch=1, device=0, paths=None,
                 preFilterCap=0, mode=None, cost=COST_BT, census=(9, 7)):
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
        cost, census = self._check_cost(cost, census)
        self._h = C.c_void_p()
        self.params = B.SGMParams(blockSize, minDisparity, numOfDisparities, P1, P2, uniquenessRatio, speckleWindowSize,
                                  speckleRange, disp12MaxDiff, paths)
        self.width, self.height, self.max_batch, self.device = width, height, max_batch, device
        B.check(B.lib().rtdm_sgm_create(C.byref(self.params), width, height, max_batch, device, C.byref(self._h)),
                "rtdm_sgm_create")
        self._created_paths = paths         # what create_right_matcher creates with, whatever setMode has said since
        self.preFilterCap = 0
        try:
            if preFilterCap:
                self.setPreFilterCap(preFilterCap)
            if cost != self.COST_BT:
                self.setCost(cost, census)
        except B.RtdmError:
            self.close()
            raise

    @classmethod
    def _check_cost(cls, cost, census):
        """-> (cost, (width, height)) as ints, or ValueError: the checks of rtdm_sgm_set_cost, made before the library is asked"""
        if isinstance(cost, bool) or cost not in (cls.COST_BT, cls.COST_CENSUS):
            raise ValueError("cost must be COST_BT (0) or COST_CENSUS (1); got %r" % (cost,))
        try:
            cw, ch = census
            ok = all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) for v in (cw, ch))
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise ValueError("census must be a (width, height) pair of ints; got %r" % (census,))
        if cost == cls.COST_CENSUS and (cw not in cls._CENSUS_W or ch not in cls._CENSUS_H):
            raise ValueError("census window must be width 3, 5, 7 or 9 by height 3, 5 or 7; got %r" % (census,))
        return int(cost), (int(cw), int(ch))

    def setCost(self, cost, census=(9, 7)):
        """The pixel cost from the next compute call on: COST_BT, or COST_CENSUS over a census = (width, height) window
        (rtdm_sgm_set_cost; COST_BT ignores census).  preFilterCap stays stored and has no effect under COST_CENSUS."""
        cost, (cw, ch) = self._check_cost(cost, census)
        B.check(B.lib().rtdm_sgm_set_cost(self._h, cost, cw, ch), "rtdm_sgm_set_cost")

    def getCost(self):
        """-> (cost, (width, height)); the window is that of the last census setting, (9, 7) before the first"""
        c, w, h = C.c_int(), C.c_int(), C.c_int()
        B.check(B.lib().rtdm_sgm_get_cost(self._h, C.byref(c), C.byref(w), C.byref(h)), "rtdm_sgm_get_cost")
        return c.value, (w.value, h.value)

    def setMode(self, mode):
        """cv::StereoSGBM::setMode on the live matcher, from the next compute call on (rtdm_sgm_set_mode): MODE_SGBM, MODE_HH,
        MODE_HH4 or MODE_SGBM_3WAY -- the one door to the last (rules T1-T8; numOfDisparities <= 256).
        The mode property and params.paths follow it."""
        if isinstance(mode, bool) or not isinstance(mode, (int, np.integer)) or int(mode) not in self._MODE_PATHS:
            raise ValueError("mode must be MODE_SGBM (0), MODE_HH (1), MODE_SGBM_3WAY (2) or MODE_HH4 (3); got %r" % (mode,))
        mode = int(mode)
        B.check(B.lib().rtdm_sgm_set_mode(self._h, mode), "rtdm_sgm_set_mode")
        self.params.paths = self._MODE_PATHS[mode]

    def getMode(self):
        """cv::StereoSGBM::getMode, as the library holds it (rtdm_sgm_get_mode)"""
        v = C.c_int()
        B.check(B.lib().rtdm_sgm_get_mode(self._h, C.byref(v)), "rtdm_sgm_get_mode")
        return v.value

    def setPreFilterCap(self, preFilterCap):
        """cv::StereoSGBM::setPreFilterCap: applies from the next compute call; >= 128 is refused (RTDM_ERR_UNSUPPORTED)."""
        B.check(B.lib().rtdm_sgm_set_prefilter_cap(self._h, int(preFilterCap)), "rtdm_sgm_set_prefilter_cap")
        self.preFilterCap = int(preFilterCap)

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
        """the path-pass form of the last call: "sweep", "vert", "half", "wide_w1", "wide_w4", "vert3" -- rtdm_sgm_path_variant"""
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
        # (the mode is not part of what rtdm_sgm_right_params carries over: created as the left one was, then set as it is set)
        r = HIPSemiGlobalMatcher(blockSize=rp.blockSize, minDisparity=rp.minDisparity, numOfDisparities=rp.numDisparities,
                                 uniquenessRatio=rp.uniquenessRatio, speckleWindowSize=rp.speckleWindowSize,
                                 speckleRange=rp.speckleRange, disp12MaxDiff=rp.disp12MaxDiff, P1=rp.P1, P2=rp.P2,
                                 width=m.width, height=m.height, max_batch=m.max_batch, device=m.device, paths=m._created_paths,
                                 preFilterCap=m.preFilterCap, cost=m.getCost()[0], census=m.getCost()[1])
        if m.params.paths != m._created_paths:
            try:
                r.setMode(m.mode)
            except B.RtdmError:
                r.close()
                raise
        return r
    raise ValueError("create_right_matcher takes a HIPMatcher or a HIPSemiGlobalMatcher; got %s" % type(m).__name__)
