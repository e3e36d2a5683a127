"""StereoSGBM with the census pixel cost (rtdm_sgm_set_cost, rules N1-N5 of DESIGN.md section 4.20): the reference the GPU tests
compare against.  The cost is the project's own -- cv::StereoSGBM has none like it, so there is no library to be at parity with.

Only the pixel cost changes, so this file states N1 (the descriptor) and N2 (the Hamming cost) in NumPy and chains every later
stage as sgm_hh4_ref.py chains it: orc_sgm_block_cost, then orc_sgm_aggregate_paths for 5 / 8 paths or sgm_hh4_ref.aggregate
for 4, then sgm_hh4_ref.finish (selection, median, speckle filter) -- including the W1 <= 0 early return and the refusal of a
frame whose block cost + P2 passes 32767 (N4).

  N1  descriptor of (x, y) over an odd window cw x ch (cw in 3, 5, 7, 9; ch in 3, 5, 7): one bit per offset (i, j) != (0, 0),
      |i| <= cw / 2, |j| <= ch / 2: I[clamp(y + j, 0, H - 1)][clamp(x + i, 0, W - 1)] < I[y][x], strict.  At most 62 bits.
  N2  cost(x, y, d) = popcount(cL(x, y) xor cR(x - d - minD, y)) <= M = cw ch - 1 on the column domain
      [max(minD + D, 0), W + min(minD, 0))
  N3  no ftzero, no overwritten border columns, preFilterCap without effect
"""
import ctypes as C

import numpy as np

import sgm_hh4_ref
from sgm_cn_ref import CostOverflow          # noqa: F401  (re-exported)

WIDTHS, HEIGHTS = (3, 5, 7, 9), (3, 5, 7)


def offsets(cw, ch):
    """the (i, j) of the descriptor's bits, bit 0 first"""
    assert cw in WIDTHS and ch in HEIGHTS
    return [(i, j) for j in range(-(ch // 2), ch // 2 + 1) for i in range(-(cw // 2), cw // 2 + 1) if (i, j) != (0, 0)]


def descriptors(img, cw, ch):
    """N1 -> uint64 [H, W]"""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 2
    H, W = img.shape
    ys, xs = np.arange(H), np.arange(W)
    out = np.zeros((H, W), np.uint64)
    for bit, (i, j) in enumerate(offsets(cw, ch)):
        nb = img[np.clip(ys + j, 0, H - 1)][:, np.clip(xs + i, 0, W - 1)]
        out |= (nb < img).astype(np.uint64) << np.uint64(bit)
    return out


def popcount64(a):
    a = np.ascontiguousarray(a, np.uint64)
    return np.unpackbits(a.view(np.uint8).reshape(a.shape + (8,)), axis=-1).sum(axis=-1, dtype=np.uint16)


def pixel_cost(left, right, minDisparity, numDisparities, cw, ch):
    """N2 for a gray uint8 pair -> uint16 [H, W1, D] on the column domain"""
    H, W = left.shape
    D, minD = numDisparities, minDisparity
    x0, x1 = max(minD + D, 0), W + min(minD, 0)
    W1 = x1 - x0
    out = np.zeros((H, max(W1, 0), D), np.uint16)
    if W1 <= 0:
        return out
    cl, cr = descriptors(left, cw, ch), descriptors(right, cw, ch)
    xs = np.arange(x0, x1)
    for d in range(D):
        out[:, :, d] = popcount64(cl[:, xs] ^ cr[:, xs - (d + minD)])
    return out


def block_costs(left, right, p, census):
    """-> (C uint16 [H, W1, D], largest block cost)"""
    from oracle import oracle as orc
    L = orc.lib()
    H, W = left.shape
    D, minD = p.numDisparities, p.minDisparity
    W1 = (W + min(minD, 0)) - max(minD + D, 0)
    pix = np.ascontiguousarray(pixel_cost(left, right, minD, D, *census))
    Cc = np.zeros_like(pix)
    cmax = L.orc_sgm_block_cost(sgm_hh4_ref._p(pix, C.c_uint16), W1, H, D, p.blockSize, sgm_hh4_ref._p(Cc, C.c_uint16))
    return Cc, cmax


def aggregate(Cc, P1, P2, paths):
    """R4 + R5: the C oracle's recurrence for 5 / 8 paths, sgm_hh4_ref's for 4"""
    if paths == 4:
        return sgm_hh4_ref.aggregate(Cc, P1, P2, sgm_hh4_ref.DIRS[4])
    from oracle import oracle as orc
    H, W1, D = Cc.shape
    S = np.zeros_like(Cc)
    orc.lib().orc_sgm_aggregate_paths(sgm_hh4_ref._p(Cc, C.c_uint16), W1, H, D, P1, P2, 5 if paths == 5 else 8,
                                      sgm_hh4_ref._p(S, C.c_uint16))
    return S


def sgm_compute(left, right, census=(9, 7), **kw):
    """What the device computes for a gray pair on a census handle (paths = 8 unless given).  Raises CostOverflow where the
    device refuses the frame."""
    from oracle import oracle as orc
    left = np.ascontiguousarray(left, np.uint8); right = np.ascontiguousarray(right, np.uint8)
    assert left.shape == right.shape and left.ndim == 2                       # N5
    H, W = left.shape
    p = kw.pop("params", None) or orc.make_sgm_params(**kw)
    D, minD = p.numDisparities, p.minDisparity
    W1 = (W + min(minD, 0)) - max(minD + D, 0)
    if W1 <= 0:
        return np.full((H, W), (minD - 1) * 16, np.int16)
    P1 = p.P1 if p.P1 > 0 else 2
    P2 = max(p.P2 if p.P2 > 0 else 5, P1 + 1)
    Cc, cmax = block_costs(left, right, p, census)
    if cmax + P2 > 32767:
        raise CostOverflow("largest block cost %d + P2 %d > 32767" % (cmax, P2))
    return sgm_hh4_ref.finish(aggregate(Cc, P1, P2, p.paths), W, H, p)
