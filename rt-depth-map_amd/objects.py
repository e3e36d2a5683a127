"""The colour-class object detector over rtdm_objects_* (csrc/api_objects.hip)."""
import ctypes as C

import numpy as np

from . import binding as B
from ._marshal import Handle, device_plane, label_planes, mask_planes, object_lists, object_tuples, rgb_batch, stats_lists
from .morph import _get_morph, _morph_element

HSV_LOW, HSV_HIGH = (0, 150, 0), (9, 255, 255)          # the reference's red filter, estimator.cpp:110-115


def _hsv_range(low, high):
    return B.HsvRange((C.c_int * 3)(*[int(v) for v in low]), (C.c_int * 3)(*[int(v) for v in high]))


OBJECT_DTYPE = np.dtype([(n, "<i4") for n in ("x", "y", "width", "height", "cls", "first_pixel")] + [("reserved", "<i4", (2,))])   # rtdm_object


STATS_DTYPE = np.dtype([(n, "<i8") for n in ("m00", "m10", "m01", "m20", "m11", "m02")])   # rtdm_object_stats


def centroids(stats):
    """STATS_DTYPE records of any shape -> float64 [..., 2]: (m10 / m00, m01 / m00), NaN where m00 is 0."""
    stats = np.asarray(stats)
    if stats.dtype != STATS_DTYPE:
        raise ValueError("stats must be STATS_DTYPE records; got %s" % stats.dtype)
    m00 = stats["m00"].astype(np.float64)
    out = np.full(stats.shape + (2,), np.nan)
    ok = m00 != 0
    out[..., 0][ok] = stats["m10"][ok] / m00[ok]
    out[..., 1][ok] = stats["m01"][ok] / m00[ok]
    return out


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


class HIPObjectDetector(Handle):
    """estimator.cpp:40-53 on the device: HSV threshold -> morphological filter -> external components -> boxes.  The filter
    is the reference's open + close with the 10x10 ellipse unless set_op chose another (as HIPMorphologicalFilter.set_op).
    max_batch frames x max_classes colour classes go through one launch of the batched calls (detect_classes, detect_device)."""
    _destroy = "rtdm_objects_destroy"

    def __init__(self, width, height, device=0, max_batch=1, max_classes=1):
        self.width, self.height, self.max_batch, self.max_classes = width, height, max_batch, max_classes
        self._h = C.c_void_p()
        B.check(B.lib().rtdm_objects_create_batch(width, height, max_batch, max_classes, device, C.byref(self._h)),
                "rtdm_objects_create_batch")

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
        rgbs = rgb_batch(np.asarray(rgbs), self.height, self.width, "rgbs")
        rng, cls, nr, K = _hsv_classes(ranges, classes)
        n, H, W = rgbs.shape[0], self.height, self.width
        objs = np.zeros((n, capacity), OBJECT_DTYPE)
        counts = np.zeros((n, max(K, 1)), np.int32); rois = np.zeros((n, 4), np.int32)
        masks = np.empty((n, max(K, 1), H, W), np.uint8) if want_masks else None
        B.check(B.lib().rtdm_objects_detect_batch(self._h, n, rgbs.ctypes.data, rgbs.strides[1], rgbs.strides[0], rng, cls, nr, K,
                                                  int(min_area), int(zero_border), masks.ctypes.data if want_masks else None, W, W * H,
                                                  objs.ctypes.data, capacity, counts.ctypes.data, rois.ctypes.data),
                "rtdm_objects_detect_batch")
        out = [object_tuples(objs[f, :min(int(counts[f].sum()), capacity)]) for f in range(n)]
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
        rp, rpitch, rframe = device_plane(d_rgb, "d_rgb", torch.uint8)
        n, H, W = d_rgb.shape[0], self.height, self.width
        capacity = object_lists(d_objects, d_counts, n, K, capacity)
        if d_rois.dtype != torch.int32 or tuple(d_rois.shape) != (n, 4) or not d_rois.is_contiguous():
            raise ValueError("d_rois must be a contiguous int32 tensor n x 4")
        mp, mpitch, mplane = mask_planes(d_masks, n, K, H, W) if d_masks is not None else (None, 0, 0)
        B.check(B.lib().rtdm_objects_detect_device(self._h, n, rp, rpitch, rframe, rng, cls, nr, K, int(min_area), int(zero_border),
                                                   mp, mpitch, mplane, d_objects.data_ptr(), capacity, d_counts.data_ptr(),
                                                   d_rois.data_ptr(), stream), "rtdm_objects_detect_device")

    def detect_labels(self, rgbs, ranges, classes=None, min_area=100, zero_border=True, capacity=256, want_masks=True,
                      want_labels=True, want_stats=True):
        """detect_classes with the pixels of every object (rules L1-L4) -> (objects, rois, counts, masks, labels, stats).
        labels: int32 n x nclasses x H x W, 1 + the index in the frame's stored list on the pixels of that object's component
        and 0 everywhere else; stats: per frame the STATS_DTYPE records (raw moments over exactly the labelled pixels) of its
        stored objects -- centroids(stats[f]) gives (x, y).  masks / labels / stats are None when not wanted."""
        rgbs = rgb_batch(np.asarray(rgbs), self.height, self.width, "rgbs")
        rng, cls, nr, K = _hsv_classes(ranges, classes)
        n, H, W = rgbs.shape[0], self.height, self.width
        capacity = int(capacity)
        if capacity < 0:
            raise ValueError("capacity must not be negative; got %d" % capacity)
        objs = np.zeros((n, capacity), OBJECT_DTYPE)
        counts = np.zeros((n, max(K, 1)), np.int32); rois = np.zeros((n, 4), np.int32)
        masks = np.empty((n, max(K, 1), H, W), np.uint8) if want_masks else None
        labels = np.zeros((n, max(K, 1), H, W), np.int32) if want_labels else None
        stats = np.zeros((n, capacity), STATS_DTYPE) if want_stats else None
        B.check(B.lib().rtdm_objects_detect_labels_batch(self._h, n, rgbs.ctypes.data, rgbs.strides[1], rgbs.strides[0], rng, cls, nr, K,
                                                         int(min_area), int(zero_border), masks.ctypes.data if want_masks else None,
                                                         W, W * H, objs.ctypes.data, capacity, counts.ctypes.data, rois.ctypes.data,
                                                         labels.ctypes.data if want_labels else None, 4 * W, 4 * W * H,
                                                         stats.ctypes.data if want_stats else None),
                "rtdm_objects_detect_labels_batch")
        stored = [min(int(counts[f].sum()), capacity) for f in range(n)]
        out = [object_tuples(objs[f, :stored[f]]) for f in range(n)]
        return (out, [tuple(int(v) for v in r) for r in rois], counts, masks, labels,
                [stats[f, :stored[f]].copy() for f in range(n)] if want_stats else None)

    def detect_labels_device(self, d_rgb, ranges, classes, d_objects, d_counts, d_rois, d_masks=None, d_labels=None, d_stats=None,
                             min_area=100, zero_border=True, capacity=None, stream=None):
        """detect_device with two more optional outputs (rules L1-L4): d_labels int32 [n, nclasses, H, W] (row pitch and plane
        stride free) and d_stats uint8 [n, capacity * 48] (frame i's moments in row i; view a host copy as STATS_DTYPE; written
        for the stored objects only).  Enqueued on `stream`, not synchronised."""
        import torch
        rng, cls, nr, K = _hsv_classes(ranges, classes)
        if d_rgb.dtype != torch.uint8 or d_rgb.dim() != 4 or tuple(d_rgb.shape[1:]) != (self.height, self.width, 3):
            raise ValueError("d_rgb must be uint8 n x %d x %d x 3; got %s %s" % (self.height, self.width, d_rgb.dtype, tuple(d_rgb.shape)))
        rp, rpitch, rframe = device_plane(d_rgb, "d_rgb", torch.uint8)
        n, H, W = d_rgb.shape[0], self.height, self.width
        capacity = object_lists(d_objects, d_counts, n, K, capacity)
        if d_rois.dtype != torch.int32 or tuple(d_rois.shape) != (n, 4) or not d_rois.is_contiguous():
            raise ValueError("d_rois must be a contiguous int32 tensor n x 4")
        mp, mpitch, mplane = mask_planes(d_masks, n, K, H, W) if d_masks is not None else (None, 0, 0)
        lp, lpitch, lplane = label_planes(d_labels, n, K, H, W) if d_labels is not None else (None, 0, 0)
        sp = stats_lists(d_stats, n, capacity) if d_stats is not None else None
        B.check(B.lib().rtdm_objects_detect_labels_device(self._h, n, rp, rpitch, rframe, rng, cls, nr, K, int(min_area),
                                                          int(zero_border), mp, mpitch, mplane, d_objects.data_ptr(), capacity,
                                                          d_counts.data_ptr(), d_rois.data_ptr(), lp, lpitch, lplane, sp, stream),
                "rtdm_objects_detect_labels_device")
