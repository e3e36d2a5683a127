"""The chained calls across handles: the estimator's loop body and the depth statistics (csrc/api_chain.hip)."""
import ctypes as C

import numpy as np

from . import binding as B
from ._marshal import (Handle, device_plane, label_planes, mask_planes, measure_lists, measure_params, object_lists, object_tuples, q16,
                       regions_array, rgb_batch)
from .objects import HSV_HIGH, HSV_LOW, OBJECT_DTYPE, _hsv_classes, _hsv_range


def estimate_frame(matcher, rectifier, detector, rgb_left, rgb_right, Q, low=HSV_LOW, high=HSV_HIGH, min_area=100,
                   zero_border=True, calibration_unit=25.0, max_boxes=64, want_disp=False):
    """One iteration of Estimator::run (estimator.cpp:29-77) without capture/decode/drawing:
    -> (boxes, mean_cm, counts[, disp])."""
    rectifier._check_rgb(rgb_left); rectifier._check_rgb(rgb_right)
    rw, rh = rectifier.roi[2], rectifier.roi[3]
    boxes = (B.Region * max_boxes)(); n = C.c_int()
    mean = np.zeros(max_boxes, np.float64); cnt = np.zeros(max_boxes, np.int32)
    disp = np.empty((rh, rw), np.int16) if want_disp else None
    rng = _hsv_range(low, high)
    B.check(B.lib().rtdm_estimate_frame(matcher._h, rectifier._h, detector._h, rgb_left.ctypes.data, rgb_left.strides[0],
                                        rgb_right.ctypes.data, rgb_right.strides[0], q16(Q),
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
    disp = np.empty((rh, rw), np.int16) if want_disp else None
    rng, cls, nr, K = _hsv_classes(ranges, classes)
    B.check(B.lib().rtdm_estimate_frame_classes(matcher._h, rectifier._h, detector._h, rgb_left.ctypes.data, rgb_left.strides[0],
                                                rgb_right.ctypes.data, rgb_right.strides[0], q16(Q),
                                                rng, cls, nr, K, int(min_area), int(zero_border), calibration_unit, objs.ctypes.data,
                                                mean.ctypes.data_as(C.POINTER(C.c_double)), cnt.ctypes.data_as(C.POINTER(C.c_int)),
                                                max_objects, C.byref(n), disp.ctypes.data if want_disp else None, rw * 2),
            "rtdm_estimate_frame_classes")
    k = min(n.value, max_objects)
    out = object_tuples(objs[:k])
    k = min(k, B.MAX_REGIONS)
    return (out, mean[:k], cnt[:k], disp) if want_disp else (out, mean[:k], cnt[:k])


def depth_stats_device(d_disp, Q, d_mask, regions, calibration_unit=25.0, device=0, stream=None):
    """torch CUDA tensors: int16 [H,W] x16 disparity, uint8 [H,W] mask -> (mean_cm[n], counts[n]); synchronous."""
    H, W = d_disp.shape
    n = len(regions)
    mean = np.zeros(n, np.float64); cnt = np.zeros(n, np.int32)
    B.check(B.lib().rtdm_depth_stats_device(device, d_disp.data_ptr(), W * 2, W, H, q16(Q),
                                            d_mask.data_ptr(), W, regions_array(regions), n, calibration_unit,
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
    return _depth_objects(False, d_disp, Q, d_masks, d_objects, d_counts, d_mean_cm, d_npix, calibration_unit, capacity, d_workspace,
                          device, stream)


def depth_objects_labels_device(d_disp, Q, d_labels, d_objects, d_counts, d_mean_cm, d_npix, calibration_unit=25.0, capacity=None,
                                d_workspace=None, device=0, stream=None):
    """depth_objects_device over every object's OWN pixels (rtdm_depth_objects_labels_device, rule L5): d_labels int32
    [n, nclasses, H, W] as HIPObjectDetector.detect_labels_device leaves them (row pitch and plane stride free) in place of the
    class masks; everything else as depth_objects_device.  -> the workspace tensor."""
    return _depth_objects(True, d_disp, Q, d_labels, d_objects, d_counts, d_mean_cm, d_npix, calibration_unit, capacity, d_workspace,
                          device, stream)


def _depth_objects(labels, d_disp, Q, d_masks, d_objects, d_counts, d_mean_cm, d_npix, calibration_unit, capacity, d_workspace, device,
                   stream):
    """Both forms of the call: the planes are the class masks (uint8) or the detector's label planes (int32)."""
    import torch
    dp, dpitch, dframe = device_plane(d_disp, "d_disp", torch.int16)
    n, H, W = d_disp.shape
    K = d_masks.shape[1] if d_masks.dim() == 4 else 0          # the class count is the masks'; any other rank is refused below
    mp, mpitch, mplane = (label_planes if labels else mask_planes)(d_masks, n, K, H, W)
    capacity = object_lists(d_objects, d_counts, n, K, capacity)
    if d_mean_cm.dtype != torch.float64 or tuple(d_mean_cm.shape) != (n, capacity) or not d_mean_cm.is_contiguous():
        raise ValueError("d_mean_cm must be a contiguous float64 tensor n x capacity")
    if d_npix.dtype != torch.int32 or tuple(d_npix.shape) != (n, capacity) or not d_npix.is_contiguous():
        raise ValueError("d_npix must be a contiguous int32 tensor n x capacity")
    need = depth_objects_workspace_bytes(n, capacity, H)
    if d_workspace is None:
        d_workspace = torch.empty(need, dtype=torch.uint8, device=d_disp.device)
    name = "rtdm_depth_objects_labels_device" if labels else "rtdm_depth_objects_device"
    B.check(getattr(B.lib(), name)(device, n, dp, dpitch, dframe, W, H, q16(Q),
                                   mp, mpitch, mplane, K, d_objects.data_ptr(), capacity, d_counts.data_ptr(),
                                   calibration_unit, d_mean_cm.data_ptr(), d_npix.data_ptr(), d_workspace.data_ptr(),
                                   d_workspace.numel(), stream), name)
    return d_workspace


MEASURE_DTYPE = np.dtype([("npix", "<i4"), ("nplane", "<i4"), ("zq", "<f4", (8,)), ("lo", "<f4", (3,)), ("hi", "<f4", (3,)),
                          ("mean", "<f8", (3,))])                          # rtdm_object_measure, 88 bytes


class MeasureParams:
    """What rtdm_objects_measure_device measures (rules G3-G5): the disparity mode of the points (XYZ_ROUNDED, the reference's,
    or XYZ_FIXED16, sub-pixel), calc_depth's Z limit, and up to eight quantiles of Z in permille (0 the minimum, 500 the lower
    median, 1000 the maximum; nothing is interpolated).  The defaults are rtdm_measure_default_params'."""

    def __init__(self, disparity_mode=B.XYZ_ROUNDED, max_z=1e4, permille=(500, 250, 750)):
        self.c = measure_params(disparity_mode, max_z, permille)
        self.disparity_mode, self.max_z, self.permille = self.c.disparity_mode, self.c.max_z, tuple(self.c.permille[:self.c.nquant])


def distance_cm(values, calibration_unit=25.0):
    """camera coordinates (zq, lo, hi, mean of a measurement) -> centimetres, as mean_cm: value * calibration_unit / 10"""
    return np.asarray(values, np.float64) * calibration_unit / 10.0


def objects_measure_workspace_bytes(n, capacity, height, nquant=8):
    return int(B.lib().rtdm_objects_measure_workspace_bytes(int(n), int(capacity), int(height), int(nquant)))


def objects_measure_device(d_disp, Q, d_planes, d_objects, d_counts, d_measures, params=None, labels=False, capacity=None,
                           d_workspace=None, device=0, stream=None):
    """Z quantiles, extent and centre of every object of n frames from the detector's device lists
    (rtdm_objects_measure_device, rules G1-G10).  torch device tensors: d_disp, d_objects, d_counts as depth_objects_device
    takes them; d_planes the class masks (uint8 [n, nclasses, H, W]) or, with labels=True, the detector's label planes (int32);
    d_measures uint8 [n, capacity * 88], written for the stored objects only (view a host copy as MEASURE_DTYPE).  params: a
    MeasureParams (None: the defaults).  d_workspace: a uint8 tensor of at least objects_measure_workspace_bytes(n, capacity,
    H, nquant) bytes (None: one is allocated through torch and returned; keep it until the work has finished).  Enqueued on
    `stream` (a raw hipStream_t value; None = the null stream), not synchronised.  -> the workspace tensor."""
    import torch
    params = params or MeasureParams()
    dp, dpitch, dframe = device_plane(d_disp, "d_disp", torch.int16)
    n, H, W = d_disp.shape
    K = d_planes.shape[1] if d_planes.dim() == 4 else 0
    pp, ppitch, pplane = (label_planes if labels else mask_planes)(d_planes, n, K, H, W)
    capacity = object_lists(d_objects, d_counts, n, K, capacity)
    mp = measure_lists(d_measures, n, capacity)
    if d_workspace is None:
        d_workspace = torch.empty(objects_measure_workspace_bytes(n, capacity, H, params.c.nquant), dtype=torch.uint8, device=d_disp.device)
    B.check(B.lib().rtdm_objects_measure_device(device, C.byref(params.c), n, dp, dpitch, dframe, W, H, q16(Q), pp, ppitch, pplane,
                                                int(bool(labels)), K, d_objects.data_ptr(), capacity, d_counts.data_ptr(), mp,
                                                d_workspace.data_ptr(), d_workspace.numel(), stream), "rtdm_objects_measure_device")
    return d_workspace


class HIPEstimator(Handle):
    """The loop body of Estimator::run (estimator.cpp:29-77) on frame batches: rtdm_estimate_batch.  Borrows a HIPMatcher, a
    HIPRectifier and a HIPObjectDetector (keep them alive; close this first); a chunk is min(max_batch, the matcher's, the
    detector's max_batch) frames, `capacity` objects of a frame are stored and measured."""
    _destroy = "rtdm_estimator_destroy"

    def __init__(self, matcher, rectifier, detector, max_batch=1, capacity=256, own_pixels=False, device_roi=False):
        self.matcher, self.rectifier, self.detector = matcher, rectifier, detector
        self.max_batch, self.capacity = int(max_batch), int(capacity)
        self._h = C.c_void_p()
        B.check(B.lib().rtdm_estimator_create(matcher._h, rectifier._h, detector._h, self.max_batch, self.capacity, C.byref(self._h)),
                "rtdm_estimator_create")
        if own_pixels:
            self.own_pixels = True
        if device_roi:
            self.device_roi = True

    @property
    def device_roi(self):
        """True: the matcher reads every frame's union box from device memory (rtdm_estimator_set_device_roi) -- no read-back in
        front of it; estimate_device then never synchronises.  Same outputs; the matcher's ROI1 stays as the caller set it."""
        on = C.c_int()
        B.check(B.lib().rtdm_estimator_get_device_roi(self._h, C.byref(on)), "rtdm_estimator_get_device_roi")
        return bool(on.value)

    @device_roi.setter
    def device_roi(self, on):
        B.check(B.lib().rtdm_estimator_set_device_roi(self._h, int(bool(on))), "rtdm_estimator_set_device_roi")

    @property
    def own_pixels(self):
        """True: every object is measured over its own pixels (its label), not over its class's mask inside its box (rule L7)."""
        on = C.c_int()
        B.check(B.lib().rtdm_estimator_get_own_pixels(self._h, C.byref(on)), "rtdm_estimator_get_own_pixels")
        return bool(on.value)

    @own_pixels.setter
    def own_pixels(self, on):
        B.check(B.lib().rtdm_estimator_set_own_pixels(self._h, int(bool(on))), "rtdm_estimator_set_own_pixels")

    def estimate(self, rgb_left, rgb_right, Q, ranges, classes=None, min_area=100, zero_border=True, calibration_unit=25.0,
                 want_disp=False, disp=None, measure=None):
        """rgb_left / rgb_right: n x H x W x 3 uint8 (R first; row pitch and frame stride free) -> (objects, counts, mean_cm,
        npix[, disp][, measures]): per frame the list of (x, y, w, h, cls) -- at most `capacity` --, counts n x nclasses (not
        clipped), and per frame the arrays of its stored objects' mean depth [cm] and pixel count.  disp: n x crop H x crop W
        int16; frames without objects keep what it held (zeros when it is allocated here).  measure: a MeasureParams -- the
        stored objects are also measured (rtdm_estimate_batch_measured) and the result ends with one more item, per frame the
        MEASURE_DTYPE records of its stored objects."""
        rc = self.rectifier
        rgb_left, rgb_right = (rgb_batch(np.asarray(a), rc.height, rc.width, "frames") for a in (rgb_left, rgb_right))
        if rgb_right.shape[0] != rgb_left.shape[0]:
            raise ValueError("frames must be uint8 n x %d x %d x 3; got %s %s" % (rc.height, rc.width, rgb_right.dtype, rgb_right.shape))
        n, cap = rgb_left.shape[0], self.capacity
        rw, rh = rc.roi[2], rc.roi[3]
        rng, cls, nr, K = _hsv_classes(ranges, classes)
        objs = np.zeros((n, cap), OBJECT_DTYPE); counts = np.zeros((n, max(K, 1)), np.int32)
        mean = np.zeros((n, cap), np.float64); npix = np.zeros((n, cap), np.int32)
        if want_disp and disp is None:
            disp = np.zeros((n, rh, rw), np.int16)
        if disp is not None and (disp.dtype != np.int16 or disp.shape != (n, rh, rw) or not disp.flags.c_contiguous):
            raise ValueError("disp must be a contiguous int16 array %s" % ((n, rh, rw),))
        args = (self._h, n, rgb_left.ctypes.data, rgb_left.strides[1], rgb_left.strides[0],
                rgb_right.ctypes.data, rgb_right.strides[1], rgb_right.strides[0],
                q16(Q), rng, cls, nr, K, int(min_area), int(zero_border),
                calibration_unit, objs.ctypes.data, counts.ctypes.data, mean.ctypes.data, npix.ctypes.data,
                disp.ctypes.data if disp is not None else None, rw * 2, rw * rh * 2)
        if measure is None:
            B.check(B.lib().rtdm_estimate_batch(*args), "rtdm_estimate_batch")
        else:
            meas = np.zeros((n, cap), MEASURE_DTYPE)
            B.check(B.lib().rtdm_estimate_batch_measured(*(args + (C.byref(measure.c), meas.ctypes.data))), "rtdm_estimate_batch_measured")
        out, means, pixels, records = [], [], [], []
        for f in range(n):
            k = min(int(counts[f].sum()), cap)
            out.append(object_tuples(objs[f, :k]))
            means.append(mean[f, :k].copy()); pixels.append(npix[f, :k].copy())
            if measure is not None:
                records.append(meas[f, :k].copy())
        res = (out, counts, means, pixels) + ((disp,) if disp is not None else ())
        return res + (records,) if measure is not None else res

    def estimate_device(self, d_rgb_left, d_rgb_right, Q, ranges, classes, d_objects, d_counts, d_mean_cm, d_npix, d_disp=None,
                        min_area=100, zero_border=True, calibration_unit=25.0, stream=None, d_measures=None, measure=None):
        """torch device tensors: uint8 [n,H,W,3] frames (row pitch and frame stride free); d_objects uint8 [n, capacity * 32],
        d_counts int32 [n, nclasses], d_mean_cm float64 [n, capacity], d_npix int32 [n, capacity], optional d_disp int16
        [n, crop H, crop W] (row pitch and frame stride free).  Enqueued on `stream` (a raw hipStream_t value; None = the null
        stream), which is synchronised once per chunk (with device_roi: never); the results are complete on the stream, not
        synchronised.  d_measures:
        uint8 [n, capacity * 88] -- the stored objects are also measured (rtdm_estimate_batch_measured_device) with `measure`, a
        MeasureParams (None: the defaults); view a host copy as MEASURE_DTYPE."""
        import torch
        rc, cap = self.rectifier, self.capacity
        rng, cls, nr, K = _hsv_classes(ranges, classes)
        n = d_rgb_left.shape[0]
        ptr = []
        for t, name in ((d_rgb_left, "d_rgb_left"), (d_rgb_right, "d_rgb_right")):
            if t.dim() != 4 or tuple(t.shape) != (n, rc.height, rc.width, 3):
                raise ValueError("%s must be uint8 n x %d x %d x 3; got %s" % (name, rc.height, rc.width, tuple(t.shape)))
            ptr.append(device_plane(t, name, torch.uint8))
        for t, name, dtype, shape in ((d_objects, "d_objects", torch.uint8, (n, cap * 32)), (d_counts, "d_counts", torch.int32, (n, K)),
                                      (d_mean_cm, "d_mean_cm", torch.float64, (n, cap)), (d_npix, "d_npix", torch.int32, (n, cap))):
            if t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous():
                raise ValueError("%s must be a contiguous %s tensor %s; got %s %s" % (name, dtype, shape, t.dtype, tuple(t.shape)))
        dp, dpitch, dframe = None, 0, 0
        if d_disp is not None:
            dp, dpitch, dframe = device_plane(d_disp, "d_disp", torch.int16, (n, rc.roi[3], rc.roi[2]))
        (lp, lpitch, lframe), (rp, rpitch, rframe) = ptr
        args = (self._h, n, lp, lpitch, lframe, rp, rpitch, rframe, q16(Q), rng, cls, nr, K, int(min_area), int(zero_border),
                calibration_unit, d_objects.data_ptr(), d_counts.data_ptr(), d_mean_cm.data_ptr(), d_npix.data_ptr(), dp, dpitch, dframe,
                stream)
        if d_measures is None:
            if measure is not None:
                raise ValueError("measure needs d_measures")
            B.check(B.lib().rtdm_estimate_batch_device(*args), "rtdm_estimate_batch_device")
        else:
            measure = measure or MeasureParams()
            B.check(B.lib().rtdm_estimate_batch_measured_device(*(args + (C.byref(measure.c), measure_lists(d_measures, n, cap)))),
                    "rtdm_estimate_batch_measured_device")
