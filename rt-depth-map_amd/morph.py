"""The morphological filter and its structuring elements over rtdm_morph_* (csrc/api_morph.hip)."""
import ctypes as C

import numpy as np

from . import binding as B
from ._marshal import Handle

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


class HIPMorphologicalFilter(Handle):
    """VideoFilterDevice (filter/filter.h:13-37) over rtdm_morph_*; ctor shape of mf-sw.cpp:10-17.  A new filter runs the
    reference's open + close with the 10x10 ellipse; set_op chooses any of cv::morphologyEx's operations, element and
    iteration count (rules M1-M7)."""
    _destroy = "rtdm_morph_destroy"

    def __init__(self, w, h, bpp=8, max_batch=1, device=0):
        if bpp != 8:
            raise ValueError("only 8 bpp masks are filtered (mf-sw.cpp is called with bpp=8, main.cpp:133)")
        self._h = C.c_void_p()
        self.img_width, self.img_height, self.img_bpp = w, h, bpp
        B.check(B.lib().rtdm_morph_create(w, h, max_batch, device, C.byref(self._h)), "rtdm_morph_create")

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
