"""Depth map and point cloud over rtdm_xyz_* (csrc/api_xyz.hip)."""
import ctypes as C

import numpy as np

from . import binding as B
from ._marshal import Handle, device_plane, host_plane
from .matcher import HIPMatcher

POINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("r", "u1"), ("g", "u1"), ("b", "u1"), ("a", "u1")])   # rtdm_point
XYZ_FIXED16, XYZ_ROUNDED = B.XYZ_FIXED16, B.XYZ_ROUNDED


class HIPReprojector(Handle):
    """cv::reprojectImageTo3D (estimator.cpp:76) and the point cloud of the pixels calc_depth keeps (estimator.cpp:235) over
    rtdm_xyz_* (rules X1-X8).  Q: 4x4; mode: XYZ_ROUNDED (the reference's `left_disp /= 16.`) or
    XYZ_FIXED16 (d = disp / 16.0, sub-pixel); min_disparity: the matcher's.  Disparity maps are the matchers' int16 x16 maps."""
    _destroy = "rtdm_xyz_destroy"

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
        d = host_plane(disp, np.int16, "disp")
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
            g = host_plane(guide, np.uint8, "guide", shape)
            cn = 1 if g.ndim == 2 else g.shape[2]
            if g.ndim not in (2, 3) or cn not in (1, 3):
                raise ValueError("guide must be H x W, H x W x 1 or H x W x 3; got shape %s" % (g.shape,))
        if mask is not None:
            m = host_plane(mask, np.uint8, "mask", shape)
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
        l = host_plane(left, np.uint8, "left")
        r = host_plane(right, np.uint8, "right", l.shape[:2])
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

    def map_device(self, d_disp, d_xyz=None, d_z=None, stream=None):
        """torch device tensors: int16 [n,H,W] in; float32 [n,H,W,3] and / or float32 [n,H,W] out (row pitch and frame stride
        free).  Enqueued on `stream` (a raw hipStream_t value; None = the null stream), not synchronised."""
        import torch
        if d_xyz is None and d_z is None:
            raise ValueError("map_device needs d_xyz, d_z or both")
        dp, dpitch, dframe = device_plane(d_disp, "d_disp", torch.int16)
        n, H, W = d_disp.shape[:3]
        xp = xpitch = xframe = zp = zpitch = zframe = None
        if d_xyz is not None:
            if d_xyz.dim() != 4 or d_xyz.shape[3] != 3:
                raise ValueError("d_xyz must be n x H x W x 3; got %s" % (tuple(d_xyz.shape),))
            xp, xpitch, xframe = device_plane(d_xyz, "d_xyz", torch.float32, (n, H, W))
        if d_z is not None:
            if d_z.dim() != 3:
                raise ValueError("d_z must be n x H x W; got %s" % (tuple(d_z.shape),))
            zp, zpitch, zframe = device_plane(d_z, "d_z", torch.float32, (n, H, W))
        B.check(B.lib().rtdm_xyz_map_device(self._h, n, dp, dpitch, dframe, W, H, xp, xpitch or 0, xframe or 0, zp, zpitch or 0,
                                            zframe or 0, stream), "rtdm_xyz_map_device")

    def cloud_device(self, d_disp, d_points, d_counts, d_guide=None, d_mask=None, capacity=None, stream=None):
        """torch device tensors: int16 [n,H,W] map; d_points: uint8 [n, >= capacity * 16] (frame i's records in row i; view it
        as POINT_DTYPE on the host); d_counts: int32 [n]; optional uint8 guide [n,H,W] or [n,H,W,3] and mask [n,H,W].
        capacity: records per frame, what a row of d_points holds when None.  Enqueued on `stream`, not synchronised."""
        import torch
        dp, dpitch, dframe = device_plane(d_disp, "d_disp", torch.int16)
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
            gp, gpitch, gframe = device_plane(d_guide, "d_guide", torch.uint8, (n, H, W))
        mp, mpitch, mframe = None, 0, 0
        if d_mask is not None:
            if d_mask.dim() != 3:
                raise ValueError("d_mask must be n x H x W; got %s" % (tuple(d_mask.shape),))
            mp, mpitch, mframe = device_plane(d_mask, "d_mask", torch.uint8, (n, H, W))
        B.check(B.lib().rtdm_xyz_cloud_device(self._h, n, dp, dpitch, dframe, gp, gpitch, gframe, cn, mp, mpitch, mframe, W, H,
                                              d_points.data_ptr(), d_points.stride(0), cap, d_counts.data_ptr(), stream),
                "rtdm_xyz_cloud_device")
