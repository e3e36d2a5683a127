"""StereoSGBM's MODE_HH4 (paths = 4, rule R4'): the reference the GPU tests compare against.

Only the set of path directions changes, so this file restates R4 (oracle/sgm_oracle.c) in NumPy for an ARBITRARY direction
set and chains every other stage through the C oracle's own entry points (pixel cost -- or sgm_cn_ref.pixel_cost for colour
and preFilterCap --, block cost, selection, median, speckle filter), exactly as orc_sgm_compute chains them, including its
W1 <= 0 early return and its refusal of a frame whose block cost + P2 passes 32767.  With the 5- and 8-direction sets the
NumPy R4 must equal orc_sgm_aggregate_paths byte for byte (test_sgm_hh4_cpu.py), which anchors its 4-direction output to
the oracle's recurrence.

R4': the four directions (1, 0), (-1, 0), (0, 1), (0, -1) and no others; R1-R3 and R5-R12 unchanged.  The rule restates
cv::StereoSGBM's computeDisparitySGBM_HH4 (OpenCV 3.4 / 4.x) from memory; like the rest of the oracle, parity with the library
itself is unpinned.
"""
import ctypes as C

import numpy as np

import sgm_cn_ref
from sgm_cn_ref import CostOverflow          # noqa: F401  (re-exported)

DIRS8 = ((1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, 1), (1, -1), (-1, -1))
DIRS = {4: DIRS8[:4], 5: tuple(d for d in DIRS8 if d[1] >= 0), 8: DIRS8}


def _step(prev, c, P1, P2):
    """R4 for a batch of lines: prev, c int64 [n, D] -> L_r [n, D]"""
    big = np.int64(1) << 40                                      # "d - 1 / d + 1 outside [0, D) never win"
    m = prev.min(axis=1, keepdims=True)
    dn = np.full_like(prev, big); dn[:, 1:] = prev[:, :-1] + P1
    up = np.full_like(prev, big); up[:, :-1] = prev[:, 1:] + P1
    return c + np.minimum(np.minimum(prev, m + P2), np.minimum(dn, up)) - m


def path_costs(Cc, dx, dy, P1, P2):
    """L_r of one direction over the block costs Cc (uint16 [H, W1, D]) -> int64 [H, W1, D].  Rows (or, for a horizontal
    direction, columns) are walked in path order; the pixels of one row step are independent lines."""
    H, W, D = Cc.shape
    c = Cc.astype(np.int64)
    L = np.empty_like(c)
    if dy == 0:
        xs = range(W) if dx > 0 else range(W - 1, -1, -1)
        prev = None
        for x in xs:
            L[:, x] = c[:, x] if prev is None else _step(L[:, prev], c[:, x], P1, P2)
            prev = x
        return L
    ys = range(H) if dy > 0 else range(H - 1, -1, -1)
    py = None
    for y in ys:
        if py is None:
            L[y] = c[y]
        else:
            src = np.arange(W) - dx                               # the previous pixel's column
            inside = (src >= 0) & (src < W)
            L[y] = c[y]                                           # a line starts where its predecessor is outside the domain
            if inside.any():
                L[y, inside] = _step(L[py, src[inside]], c[y, inside], P1, P2)
        py = y
    return L


def aggregate(Cc, P1, P2, dirs):
    """R4 over the direction set + R5 -> uint16 [H, W1, D]"""
    S = np.zeros(Cc.shape, np.int64)
    for dx, dy in dirs:
        S = np.minimum(S + path_costs(Cc, dx, dy, P1, P2), 32767)    # R5 (every term >= 0: grouping does not matter)
    return S.astype(np.uint16)


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def block_costs(left, right, p, preFilterCap=0):
    """-> (C uint16 [H, W1, D], largest block cost); gray at preFilterCap 0 through orc_sgm_pixel_cost, everything else through
    sgm_cn_ref.pixel_cost"""
    from oracle import oracle as orc
    L = orc.lib()
    H, W = left.shape[:2]
    D, minD = p.numDisparities, p.minDisparity
    W1 = (W + min(minD, 0)) - max(minD + D, 0)
    if left.ndim == 2 and sgm_cn_ref.ftzero(preFilterCap) == 15:
        pix = np.zeros((H, W1, D), np.uint16)
        L.orc_sgm_pixel_cost(_p(left, C.c_uint8), W, _p(right, C.c_uint8), W, W, H, minD, D, _p(pix, C.c_uint16))
    else:
        pix = np.ascontiguousarray(sgm_cn_ref.pixel_cost(left, right, minD, D, preFilterCap))
    Cc = np.zeros_like(pix)
    cmax = L.orc_sgm_block_cost(_p(pix, C.c_uint16), W1, H, D, p.blockSize, _p(Cc, C.c_uint16))
    return Cc, cmax


def finish(S, W, H, p):
    """selection, median, speckle filter: the oracle's own, as orc_sgm_compute chains them"""
    from oracle import oracle as orc
    L = orc.lib()
    D, minD = p.numDisparities, p.minDisparity
    S = np.ascontiguousarray(S, np.uint16)
    raw = np.empty((H, W), np.int16)
    L.orc_sgm_select(_p(S, C.c_uint16), W, H, D, minD, p.uniquenessRatio, p.disp12MaxDiff, _p(raw, C.c_int16), W)
    disp = np.empty((H, W), np.int16)
    L.orc_median3x3_s16(_p(raw, C.c_int16), W, _p(disp, C.c_int16), W, W, H)
    if p.speckleWindowSize > 0:
        L.orc_filter_speckles(_p(disp, C.c_int16), W, W, H, (minD - 1) * 16, p.speckleWindowSize, 16 * p.speckleRange)
    return disp


def sgm_compute(left, right, preFilterCap=0, dirs=None, **kw):
    """What the device computes for a gray or colour pair with the direction set `dirs` (default: DIRS[paths], paths = 4 unless
    given).  Raises CostOverflow where the device refuses the frame."""
    from oracle import oracle as orc
    left = np.ascontiguousarray(left, np.uint8); right = np.ascontiguousarray(right, np.uint8)
    assert left.shape == right.shape and left.ndim in (2, 3)
    H, W = left.shape[:2]
    kw.setdefault("paths", 4)
    p = kw.pop("params", None) or orc.make_sgm_params(**kw)
    if dirs is None:
        dirs = DIRS[p.paths]
    D, minD = p.numDisparities, p.minDisparity
    W1 = (W + min(minD, 0)) - max(minD + D, 0)
    if W1 <= 0:
        return np.full((H, W), (minD - 1) * 16, np.int16)
    P1 = p.P1 if p.P1 > 0 else 2
    P2 = max(p.P2 if p.P2 > 0 else 5, P1 + 1)
    Cc, cmax = block_costs(left, right, p, preFilterCap)
    if cmax + P2 > 32767:
        raise CostOverflow("largest block cost %d + P2 %d > 32767" % (cmax, P2))
    return finish(aggregate(Cc, P1, P2, dirs), W, H, p)
