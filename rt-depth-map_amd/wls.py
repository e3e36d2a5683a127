"""The WLS disparity post-filter over rtdm_wls_* (csrc/api_wls.hip)."""
import ctypes as C

import numpy as np

from . import binding as B
from ._marshal import Handle, host_plane
from .matcher import HIPMatcher, HIPSemiGlobalMatcher


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


class HIPDisparityWLSFilter(Handle):
    """cv::ximgproc::DisparityWLSFilter over rtdm_wls_* (rules W1-W8).  params: a binding.WLSParams
    (wls_params_for / create_disparity_wls_filter make it from a matcher).  filter(disparity_map_left, left_view, filtered,
    disparity_map_right) has ximgproc's call shape; the filtered map is int16 x16 with the left matcher's invalid value."""
    _destroy = "rtdm_wls_destroy"

    def __init__(self, params, width, height, max_batch=1, device=0):
        self._h = C.c_void_p()
        self.params = B.WLSParams()
        C.memmove(C.byref(self.params), C.byref(params), C.sizeof(B.WLSParams))
        self.width, self.height, self.max_batch, self.device = width, height, max_batch, device
        self.confidence_map = None
        B.check(B.lib().rtdm_wls_create(C.byref(self.params), width, height, max_batch, device, C.byref(self._h)), "rtdm_wls_create")

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
        dl = host_plane(disparity_map_left, np.int16, "disparity_map_left")
        if dl.ndim != 2:
            raise ValueError("disparity_map_left must be H x W; got shape %s" % (dl.shape,))
        H, W = dl.shape
        dr = None
        if self.params.use_confidence:
            if disparity_map_right is None:
                raise ValueError("this filter uses a confidence map: disparity_map_right is required")
            dr = host_plane(disparity_map_right, np.int16, "disparity_map_right", (H, W))
        g = host_plane(left_view, np.uint8, "left_view", (H, W))
        cn = 1 if g.ndim == 2 else g.shape[2]
        out = np.empty((H, W), np.int16) if filtered is None else host_plane(filtered, np.int16, "filtered", (H, W))
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
        l = host_plane(left, np.uint8, "left")
        r = host_plane(right, np.uint8, "right", l.shape)
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
