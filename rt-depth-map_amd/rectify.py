"""Calibration files, stereoRectify and the device rectifier over rtdm_rectify_* (csrc/api_rectify.hip)."""
import ctypes as C

import numpy as np

from . import binding as B
from ._marshal import Handle


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


class HIPRectifier(Handle):
    """estimator.cpp:29-39 on the device: RGB -> gray -> remap(INTER_LINEAR, CV_16SC2 maps) -> crop to roif.

    map1_*: HxWx2 int16, map2_*: HxW uint16 (what initUndistortRectifyMap(..., CV_16SC2, ...) returns, main.cpp:95-96);
    roi = (x, y, w, h) = the reference's roif (main.cpp:80-85)."""
    _destroy = "rtdm_rectify_destroy"

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
