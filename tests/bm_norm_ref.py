"""StereoBM with preFilterType NORMALIZED_RESPONSE: the reference the GPU tests compare against.

Only the prefilter changes (rule N6), so this file restates the normalised-response prefilter in NumPy (rules N1-N5, DESIGN.md
section 4.10) and chains every later stage through the C oracle's own entry points exactly as orc_bm_compute chains them: the
valid rectangle, the all-FILTERED early return, the SAD search over the valid rows, the left-right check on those rows, the
mask outside the rectangle, the speckle filter.

The rules restate prefilterNorm of OpenCV's stereobm.cpp from memory; like the rest of the oracle, parity with the library
itself is unpinned.  With ws = preFilterSize, r = ws // 2, ftzero = preFilterCap, integer arithmetic, >> arithmetic:
  N1  g = ws*ws // 8, scale_s = (1024 + g) // (2 g), scale_g = g * scale_s            (ws >= 91: both 0, the output is ftzero)
  N2  S(x, y) = sum of src over the (2r+1)^2 window, row and column indices clamped to the frame
  N3  n = 4 c + l + r' + u + d, neighbours clamped (so columns 0 and W-1 count c five times)
  N4  val = (n * scale_g - S * scale_s) >> 10
  N5  dst = clamp(val, -ftzero, ftzero) + ftzero, every row and every column

prefilter_norm is that closed form.  prefilter_norm_loop is a second, independent formulation: a transcription of the
library's loop as remembered (running column sums with their (ushort) casts and replicated ends, the running window sum,
the 2816-entry table).  It raises where the library would leave its table (TableIndexError) or read rows the frame does not
have (H < r), so it is only good for cross-checking where neither happens.
"""
import ctypes as C

import numpy as np

PREFILTER_NORMALIZED_RESPONSE, PREFILTER_XSOBEL = 0, 1


class TableIndexError(IndexError):
    """val + 1280 leaves the library's 2816-entry table: the library reads outside its array there"""


def scales(ws):
    g = ws * ws // 8
    scale_s = (1024 + g) // (2 * g)
    return scale_s, g * scale_s


def prefilter_norm(img, ws, cap):
    """N1-N5 in closed form: uint8 H x W -> uint8 H x W"""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 2 and ws % 2 == 1 and 5 <= ws <= 255 and 1 <= cap <= 63
    H, W = img.shape
    r = ws // 2
    scale_s, scale_g = scales(ws)
    a = img.astype(np.int64)
    p = np.pad(a, r + 1, mode="edge")                                     # p[y + r + 1, x + r + 1] = a[clamp y, clamp x]
    I = np.zeros((p.shape[0] + 1, p.shape[1] + 1), np.int64)
    I[1:, 1:] = p.cumsum(0).cumsum(1)                                      # I[i, j] = sum p[:i, :j]
    y0 = np.arange(H)[:, None] + 1; x0 = np.arange(W)[None, :] + 1        # window rows y0 .. y0 + 2r of p
    S = I[y0 + 2 * r + 1, x0 + 2 * r + 1] - I[y0, x0 + 2 * r + 1] - I[y0 + 2 * r + 1, x0] + I[y0, x0]
    c = p[r + 1:r + 1 + H, r + 1:r + 1 + W]
    n = (4 * c + p[r + 1:r + 1 + H, r:r + W] + p[r + 1:r + 1 + H, r + 2:r + 2 + W]
         + p[r:r + H, r + 1:r + 1 + W] + p[r + 2:r + 2 + H, r + 1:r + 1 + W])
    val = (n * scale_g - S * scale_s) >> 10
    return (np.clip(val, -cap, cap) + cap).astype(np.uint8)


def max_abs_val(ws):
    """the largest |val| any image can produce (the five cross pixels at one extreme, the rest at the other)"""
    scale_s, scale_g = scales(ws)
    hi = (8 * 255 * scale_g - 5 * 255 * scale_s) >> 10
    lo = (0 - (ws * ws - 5) * 255 * scale_s) >> 10
    return hi, lo


def table_safe(ws):
    """True where val + 1280 stays inside the library's table for EVERY image"""
    hi, lo = max_abs_val(ws)
    return hi + 1280 < 2816 and lo + 1280 >= 0


def prefilter_norm_loop(img, ws, cap):
    """the library's loop as remembered; raises TableIndexError / ValueError where the library would read out of bounds"""
    img = np.ascontiguousarray(img, np.uint8)
    H, W = img.shape
    wsz2 = ws // 2
    if H < wsz2:
        raise ValueError("the library's initial column sums read rows 1 .. %d of a frame of %d rows" % (wsz2 - 1, H))
    scale_g = ws * ws // 8
    scale_s = (1024 + scale_g) // (scale_g * 2)
    scale_g *= scale_s
    OFS = 256 * 5
    TABSZ = OFS * 2 + 256
    t = np.arange(TABSZ) - OFS
    tab = np.where(t < -cap, 0, np.where(t > cap, cap * 2, t + cap)).astype(np.uint8)
    src = img.astype(np.int64)
    U = 0xffff                                                             # the (ushort) casts
    vsum = (src[0] * (wsz2 + 2)) & U
    for y in range(1, wsz2):
        vsum = (vsum + src[y]) & U
    dst = np.empty((H, W), np.uint8)
    for y in range(H):
        top = src[max(y - wsz2 - 1, 0)]
        bottom = src[min(y + wsz2, H - 1)]
        prev = src[max(y - 1, 0)]
        curr = src[y]
        nxt = src[min(y + 1, H - 1)]
        vsum = (vsum + bottom - top) & U
        v = np.concatenate([np.full(wsz2 + 1, vsum[0]), vsum, np.full(wsz2 + 1, vsum[W - 1])])   # v[x + wsz2 + 1] = vsum[x]
        o = wsz2 + 1
        s0 = v[o] * (wsz2 + 1) + v[o + 1:o + wsz2 + 1].sum()
        xs = np.arange(1, W)
        run = s0 + np.concatenate([[0], np.cumsum(v[o + xs + wsz2] - v[o + xs - wsz2 - 1])])      # the running window sum
        n = np.empty(W, np.int64)
        n[0] = curr[0] * 5 + curr[1] + prev[0] + nxt[0]
        n[1:W - 1] = curr[1:W - 1] * 4 + curr[0:W - 2] + curr[2:W] + prev[1:W - 1] + nxt[1:W - 1]
        n[W - 1] = curr[W - 1] * 5 + curr[W - 2] + prev[W - 1] + nxt[W - 1]
        idx = ((n * scale_g - run * scale_s) >> 10) + OFS
        if idx.min() < 0 or idx.max() >= TABSZ:
            raise TableIndexError("row %d: table index %d .. %d" % (y, idx.min(), idx.max()))
        dst[y] = tab[idx]
    return dst


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def bm_chain(left, right, prefilter, legacy=False, **kw):
    """orc_bm_compute's chain with `prefilter(img, cap) -> uint8 plane` in place of its x-Sobel"""
    from oracle import oracle as orc
    left = np.ascontiguousarray(left, np.uint8); right = np.ascontiguousarray(right, np.uint8)
    assert left.shape == right.shape and left.ndim == 2
    H, W = left.shape
    p = kw.pop("params", None) or orc.make_params(**kw)
    D, minD, w = p.numDisparities, p.minDisparity, p.blockSize
    assert 1 <= p.preFilterCap <= 63 and w % 2 == 1 and 5 <= w <= 255 and w < min(W, H) and D > 0 and D % 16 == 0
    FILTERED = (minD - 1) * 16
    lofs, rofs = max(D - 1 + minD, 0), -min(D - 1 + minD, 0)
    width1 = W - rofs - D + 1
    rect = orc.valid_rect(W, H, params=p)
    disp = np.full((H, W), FILTERED, np.int16)
    if lofs >= W or rofs >= W or width1 < 1 or rect is None:
        return disp
    Lp = np.ascontiguousarray(prefilter(left, p.preFilterCap))
    Rp = np.zeros(W * H + D, np.uint8)                    # + D zeros: the legacy clamp (H1) over-reads the last row
    Rp[:W * H] = np.ascontiguousarray(prefilter(right, p.preFilterCap)).reshape(-1)
    cost = np.zeros((H, W), np.int32)
    vy0, vy1 = rect[1], rect[1] + rect[3]
    L = orc.lib()
    orc.set_legacy_right_clamp(bool(legacy))
    try:
        L.orc_bm_search(C.byref(p), _p(Lp, C.c_uint8), W, _p(Rp, C.c_uint8), W, W, H, vy0, vy1,
                        _p(disp, C.c_int16), W, _p(cost, C.c_int32), W)
    finally:
        orc.set_legacy_right_clamp(False)
    if p.disp12MaxDiff >= 0:
        disp[vy0:vy1] = orc.validate_disparity(disp[vy0:vy1], cost[vy0:vy1], minD, D, p.disp12MaxDiff)
    disp[vy0:vy1, :rect[0]] = FILTERED
    disp[vy0:vy1, rect[0] + rect[2]:] = FILTERED
    if p.speckleRange >= 0 and p.speckleWindowSize > 0:
        disp = orc.filter_speckles(disp, FILTERED, p.speckleWindowSize, p.speckleRange)
    return disp


def bm_compute_norm(left, right, preFilterSize, legacy=False, **kw):
    """What the device computes with preFilterType NORMALIZED_RESPONSE; kw as oracle.make_params (roi1 / roi2 included)."""
    return bm_chain(left, right, lambda img, cap: prefilter_norm(img, preFilterSize, cap), legacy=legacy, **kw)
