"""StereoSGBM with colour frames and preFilterCap: the reference the GPU tests compare against.

Only R1 (the pixel cost, oracle/sgm_oracle.c) changes, so this file restates R1 in NumPy for cn = 1 or 3 channels and any
ftzero, and chains every later stage through the C oracle's own entry points (block cost, paths, selection, median, speckle
filter), exactly as orc_sgm_compute chains them -- including its W1 <= 0 early return and its refusal of a frame whose block
cost + P2 passes 32767 (deviation (a)).

The rule restates cv::StereoSGBM's calcPixelCostBT from memory; like the rest of the oracle, parity with the library itself is
unpinned:
  ftzero = max(preFilterCap, 15) | 1
  for every channel c of each image: the x-Sobel with the rows above / below replicated, clipped to +-ftzero, + ftzero; the
  raw value; columns 0 and W-1 of all 2 cn rows overwritten with ftzero
  cost(x, d) = sum_c BT(gradient_c) + sum_c (BT(raw_c) >> 2)      (BT: the oracle's bt(), integer half-way points)
  a pixel cost is at most M = cn (2 ftzero + 63)
"""
import ctypes as C

import numpy as np


class CostOverflow(ValueError):
    """A block cost + P2 passes 32767: the frame is refused (RTDM_ERR_UNSUPPORTED on the device)."""


def ftzero(preFilterCap):
    return max(int(preFilterCap), 15) | 1


def max_pixel_cost(cn, preFilterCap):
    return cn * (2 * ftzero(preFilterCap) + 63)


def _planes(img, ftz):
    """-> (gradient, raw) int32 [cn, H, W] planes of one image, R1 borders applied"""
    a = img.astype(np.int32)
    if a.ndim == 2:
        a = a[:, :, None]
    a = np.moveaxis(a, 2, 0)                                   # [cn, H, W]
    H, W = a.shape[1:]
    up = a[:, np.r_[0, 0:H - 1] if H > 1 else [0], :]
    dn = a[:, np.r_[1:H, H - 1] if H > 1 else [0], :]
    g = np.full(a.shape, ftz, np.int32)
    if W > 2:
        def dx(p):
            return p[:, :, 2:] - p[:, :, :-2]
        g[:, :, 1:-1] = np.clip(2 * dx(a) + dx(up) + dx(dn), -ftz, ftz) + ftz
    raw = a.copy()
    raw[:, :, 0] = ftz
    raw[:, :, W - 1] = ftz
    return g, raw


def _bt_bounds(p):
    """Birchfield-Tomasi (value, min, max) of every column: half-way points (v + neighbour) // 2, none beyond the row ends"""
    left = p.copy(); right = p.copy()
    left[..., 1:] = (p[..., 1:] + p[..., :-1]) // 2
    right[..., :-1] = (p[..., :-1] + p[..., 1:]) // 2
    return p, np.minimum(np.minimum(left, right), p), np.maximum(np.maximum(left, right), p)


def pixel_cost(left, right, minDisparity, numDisparities, preFilterCap=0):
    """R1 for gray (H x W) or interleaved colour (H x W x 3) uint8 pairs -> uint16 [H, W1, D] on the column domain"""
    ftz = ftzero(preFilterCap)
    H, W = left.shape[:2]
    D, minD = numDisparities, minDisparity
    x0, x1 = max(minD + D, 0), W + min(minD, 0)
    W1 = x1 - x0
    out = np.zeros((H, max(W1, 0), D), np.int64)
    if W1 <= 0:
        return out.astype(np.uint16)
    gl, il = _planes(left, ftz)
    gr, ir = _planes(right, ftz)
    xs = np.arange(x0, x1)
    for planes_l, planes_r, shift in ((gl, gr, 0), (il, ir, 2)):
        u, u0, u1 = (b[:, :, xs] for b in _bt_bounds(planes_l))
        vb = _bt_bounds(planes_r)
        for d in range(D):
            xr = xs - (d + minD)
            v, v0, v1 = (b[:, :, xr] for b in vb)
            c0 = np.maximum(0, np.maximum(u - v1, v0 - u))
            c1 = np.maximum(0, np.maximum(v - u1, u0 - v))
            out[:, :, d] += (np.minimum(c0, c1) >> shift).sum(axis=0)
    return out.astype(np.uint16)


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def sgm_compute_cn(left, right, preFilterCap=0, **kw):
    """What the device computes for a gray or colour pair: R1 above, then the oracle's stages as orc_sgm_compute chains them.
    Raises CostOverflow where the device refuses the frame."""
    from oracle import oracle as orc
    left = np.ascontiguousarray(left, np.uint8); right = np.ascontiguousarray(right, np.uint8)
    assert left.shape == right.shape and left.ndim in (2, 3)
    H, W = left.shape[:2]
    p = kw.pop("params", None) or orc.make_sgm_params(**kw)
    D, minD = p.numDisparities, p.minDisparity
    INVALID = (minD - 1) * 16
    W1 = (W + min(minD, 0)) - max(minD + D, 0)
    if W1 <= 0:
        return np.full((H, W), INVALID, np.int16)
    P1 = p.P1 if p.P1 > 0 else 2
    P2 = max(p.P2 if p.P2 > 0 else 5, P1 + 1)
    L = orc.lib()
    pix = np.ascontiguousarray(pixel_cost(left, right, minD, D, preFilterCap))
    Cc = np.zeros_like(pix)
    cmax = L.orc_sgm_block_cost(_p(pix, C.c_uint16), W1, H, D, p.blockSize, _p(Cc, C.c_uint16))
    if cmax + P2 > 32767:
        raise CostOverflow("largest block cost %d + P2 %d > 32767" % (cmax, P2))
    S = np.zeros_like(pix)
    L.orc_sgm_aggregate_paths(_p(Cc, C.c_uint16), W1, H, D, P1, P2, 5 if p.paths == 5 else 8, _p(S, C.c_uint16))
    raw = np.empty((H, W), np.int16)
    L.orc_sgm_select(_p(S, C.c_uint16), W, H, D, minD, p.uniquenessRatio, p.disp12MaxDiff, _p(raw, C.c_int16), W)
    disp = np.empty((H, W), np.int16)
    L.orc_median3x3_s16(_p(raw, C.c_int16), W, _p(disp, C.c_int16), W, W, H)
    if p.speckleWindowSize > 0:
        L.orc_filter_speckles(_p(disp, C.c_int16), W, W, H, INVALID, p.speckleWindowSize, 16 * p.speckleRange)
    return disp
