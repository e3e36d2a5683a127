"""What the handle modules share: the base of the handle classes and the argument checks in front of the C ABI."""
import ctypes as C

import numpy as np

from . import binding as B


class Handle:
    """Owns the rtdm_*_create result in `_h`; `_destroy` names the entry that frees it."""
    _destroy = None

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            try:
                getattr(B.lib(), self._destroy)(self._h)
            except (TypeError, AttributeError):       # interpreter shutdown: the module globals are already gone
                pass
            self._h = None

    __del__ = close


def host_plane(a, dtype, name, shape=None):
    if not isinstance(a, np.ndarray):
        raise TypeError("%s must be a numpy array" % name)
    if a.dtype != dtype:
        raise ValueError("%s must be %s; got %s" % (name, np.dtype(dtype).name, a.dtype))
    if shape is not None and a.shape[:2] != shape:
        raise ValueError("%s has shape %s; expected %s" % (name, a.shape, shape))
    if a.strides[1] != a.itemsize * (a.shape[2] if a.ndim == 3 else 1) or (a.ndim == 3 and a.strides[2] != a.itemsize):
        raise ValueError("%s rows must be contiguous; got strides %s" % (name, a.strides))
    return a


def device_plane(t, name, dtype, shape=None):
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


def q16(Q):
    """the 4 x 4 matrix as 16 contiguous doubles -> their POINTER(c_double), which keeps the array alive"""
    return np.ascontiguousarray(Q, np.float64).reshape(16).ctypes.data_as(C.POINTER(C.c_double))


def regions_array(regions):
    """[(x, y, w, h)] -> a Region array (one entry long when the list is empty)"""
    return (B.Region * max(len(regions), 1))(*[B.Region(*[int(v) for v in r]) for r in regions])


def object_tuples(o):
    """a 1-D slice of OBJECT_DTYPE records -> [(x, y, w, h, cls)]"""
    return list(zip(o["x"].tolist(), o["y"].tolist(), o["width"].tolist(), o["height"].tolist(), o["cls"].tolist()))


def rgb_batch(a, H, W, name):
    """a host batch of interleaved colour frames, n x H x W x 3 uint8 (row pitch and frame stride free)"""
    if a.dtype != np.uint8 or a.ndim != 4 or a.shape[1:] != (H, W, 3):
        raise ValueError("%s must be uint8 n x %d x %d x 3; got %s %s" % (name, H, W, a.dtype, a.shape))
    if a.strides[2] != 3 or a.strides[3] != 1 or a.strides[1] < 3 * W or a.strides[0] < 0:
        raise ValueError("the pixels of a row must be contiguous; got strides %s" % (a.strides,))
    return a


def object_lists(d_objects, d_counts, n, K, capacity):
    """The detector's device lists: d_objects uint8 [n, capacity * 32], d_counts int32 [n, K] -> capacity (what a row of
    d_objects holds when None)."""
    import torch
    if d_objects.dtype != torch.uint8 or d_objects.dim() != 2 or d_objects.shape[0] != n or not d_objects.is_contiguous():
        raise ValueError("d_objects must be a contiguous uint8 tensor of n rows; got %s %s" % (d_objects.dtype, tuple(d_objects.shape)))
    if capacity is None:
        capacity = d_objects.shape[1] // 32
    if capacity < 0 or capacity * 32 != d_objects.shape[1]:
        raise ValueError("rows of d_objects must hold exactly capacity * 32 bytes; got %d for capacity %d" % (d_objects.shape[1], capacity))
    if d_counts.dtype != torch.int32 or tuple(d_counts.shape) != (n, K) or not d_counts.is_contiguous():
        raise ValueError("d_counts must be a contiguous int32 tensor n x nclasses")
    return capacity


def mask_planes(d_masks, n, K, H, W):
    """(pointer, row pitch, plane stride) of the uint8 [n, K, H, W] device masks (row pitch and plane stride free)"""
    import torch
    if d_masks.dtype != torch.uint8 or tuple(d_masks.shape) != (n, K, H, W):
        raise ValueError("d_masks must be uint8 n x nclasses x H x W; got %s %s" % (d_masks.dtype, tuple(d_masks.shape)))
    st = d_masks.stride()
    if st[3] != 1 or st[2] < W or st[1] < st[2] * H or (n > 1 and st[0] != K * st[1]):
        raise ValueError("d_masks: contiguous rows and one stride from plane to plane; got strides %s" % (tuple(st),))
    return d_masks.data_ptr(), st[2], st[1]


def label_planes(d_labels, n, K, H, W):
    """(pointer, row pitch, plane stride) in bytes of the int32 [n, K, H, W] device label planes (row pitch and plane stride free)"""
    import torch
    if d_labels.dtype != torch.int32 or tuple(d_labels.shape) != (n, K, H, W):
        raise ValueError("d_labels must be int32 n x nclasses x H x W; got %s %s" % (d_labels.dtype, tuple(d_labels.shape)))
    st = d_labels.stride()
    if st[3] != 1 or st[2] < W or st[1] < st[2] * H or (n > 1 and st[0] != K * st[1]):
        raise ValueError("d_labels: contiguous rows and one stride from plane to plane; got strides %s" % (tuple(st),))
    return d_labels.data_ptr(), st[2] * 4, st[1] * 4


def measure_params(disparity_mode, max_z, permille):
    """rtdm_measure_params from checked values (rule G10's RTDM_ERR_BAD_PARAM, said here with the offending value)"""
    if disparity_mode not in (B.XYZ_FIXED16, B.XYZ_ROUNDED):
        raise ValueError("disparity_mode must be XYZ_FIXED16 (0) or XYZ_ROUNDED (1); got %r" % (disparity_mode,))
    max_z = float(max_z)
    if not np.isfinite(max_z) or max_z <= 0:
        raise ValueError("max_z must be finite and positive; got %r" % (max_z,))
    permille = [int(p) for p in permille]
    if len(permille) > 8 or any(p < 0 or p > 1000 for p in permille):
        raise ValueError("permille: at most 8 values in 0 .. 1000; got %r" % (permille,))
    return B.MeasureParams(int(disparity_mode), max_z, len(permille), (C.c_int * 8)(*permille))


def measure_lists(d_measures, n, capacity):
    """the device records: uint8 [n, capacity * 88], 8-byte aligned (view a host copy as MEASURE_DTYPE)"""
    import torch
    if d_measures.dtype != torch.uint8 or tuple(d_measures.shape) != (n, capacity * 88) or not d_measures.is_contiguous():
        raise ValueError("d_measures must be a contiguous uint8 tensor n x capacity * 88; got %s %s" % (d_measures.dtype, tuple(d_measures.shape)))
    if d_measures.data_ptr() % 8:
        raise ValueError("d_measures must be 8-byte aligned")
    return d_measures.data_ptr()


def stats_lists(d_stats, n, capacity):
    """the device moments: uint8 [n, capacity * 48] (view a host copy as STATS_DTYPE)"""
    import torch
    if d_stats.dtype != torch.uint8 or tuple(d_stats.shape) != (n, capacity * 48) or not d_stats.is_contiguous():
        raise ValueError("d_stats must be a contiguous uint8 tensor n x capacity * 48; got %s %s" % (d_stats.dtype, tuple(d_stats.shape)))
    return d_stats.data_ptr()
