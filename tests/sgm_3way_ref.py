"""StereoSGBM's MODE_SGBM_3WAY (rtdm_sgm_set_mode, rules T1-T8 of DESIGN.md section 4.21): the reference the GPU tests compare
against.  T1-T5 in NumPy; the pixel costs come from orc_sgm_pixel_cost, sgm_cn_ref.pixel_cost (colour, preFilterCap) or
sgm_census_ref.pixel_cost (census), the block costs from orc_sgm_block_cost, the recurrence from sgm_hh4_ref.path_costs (anchored
to the C oracle's in test_sgm_hh4_cpu.py), and selection, median and speckle filter from sgm_hh4_ref.finish with
disp12MaxDiff = 1 << 20, which can never reject (T6: the mode has no left-right check; what orc_sgm_select's votes decide is
then never read).

The rules restate cv::StereoSGBM's computeDisparity3WAY / SGBM3WayMainLoop (OpenCV 3.4 / 4.x) from memory; like R1-R12 and R4',
parity with the library itself is UNPINNED.

  T1  always 4 stripes; sz = (H + 3) // 4, ovl = (blockSize // 2 + 1) + (sz + 9) // 10 (the library's (int)ceil(0.1 * sz));
      stripe s: output rows [o, e) = [min(s sz, H), min((s + 1) sz, H)), first source row a = max(min(s sz - ovl, H), 0)
  T2  R1-R3 unchanged except for T3's rows
  T3  y in [a, min(a + R, e)), R = blockSize // 2: C'(y) = sum over j = -R .. R of h(clamp(y + j, a, H - 1)), h(r) = R3's horizontal
      sum of row r's pixel costs (first and last column of the domain replicated); a = 0: C' = C
  T4  (1, 0), (-1, 0) over the whole frame's C (R4); (0, 1) per stripe from row a with L = C'(a); rows [a, o) serve the recurrence only
  T5  S = min(L-> + L<- + Ldown, 32767) on the output rows
  T6  R6, R8 unchanged; no R7, no R9
  T7  R10-R12 unchanged
  T8  where M window^2 + P2 > 32767: every block cost the mode reads, every C' included, against 32767 - P2
"""
import ctypes as C

import numpy as np

import sgm_census_ref
import sgm_cn_ref
import sgm_hh4_ref
from sgm_cn_ref import CostOverflow          # noqa: F401  (re-exported)

NSTRIPES = 4
NEVER = 1 << 20                               # a disp12MaxDiff no pair of disparities can exceed


def stripes(H, blockSize, nstripes=NSTRIPES):
    """T1 -> [(a, o, e)] (nstripes other than 4: the same rule with that count, for the anchors of test_sgm_3way_cpu.py)"""
    sz = (H + nstripes - 1) // nstripes
    ovl = (blockSize // 2 + 1) + (sz + 9) // 10
    return [(max(min(s * sz - ovl, H), 0), min(s * sz, H), min((s + 1) * sz, H)) for s in range(nstripes)]


def pixel_costs(left, right, p, preFilterCap=0, census=None):
    """-> uint16 [H, W1, D], as the device's cost stage has them for this handle"""
    from oracle import oracle as orc
    H, W = left.shape[:2]
    D, minD = p.numDisparities, p.minDisparity
    W1 = (W + min(minD, 0)) - max(minD + D, 0)
    if census is not None:
        assert left.ndim == 2
        return np.ascontiguousarray(sgm_census_ref.pixel_cost(left, right, minD, D, *census))
    if left.ndim == 2 and sgm_cn_ref.ftzero(preFilterCap) == 15:
        pix = np.zeros((H, W1, D), np.uint16)
        _p = sgm_hh4_ref._p
        orc.lib().orc_sgm_pixel_cost(_p(left, C.c_uint8), W, _p(right, C.c_uint8), W, W, H, minD, D, _p(pix, C.c_uint16))
        return pix
    return np.ascontiguousarray(sgm_cn_ref.pixel_cost(left, right, minD, D, preFilterCap))


def block_costs(pix, blockSize):
    """R3 -> (C uint16 [H, W1, D], largest block cost): the oracle's own"""
    from oracle import oracle as orc
    H, W1, D = pix.shape
    Cc = np.zeros_like(pix)
    _p = sgm_hh4_ref._p
    cmax = orc.lib().orc_sgm_block_cost(_p(pix, C.c_uint16), W1, H, D, blockSize, _p(Cc, C.c_uint16))
    return Cc, int(cmax)


def row_sums(pix, blockSize):
    """h(r) of T3 -> int64 [H, W1, D]"""
    H, W1, D = pix.shape
    R = blockSize // 2
    p = pix.astype(np.int64)
    xs = np.arange(W1)
    return sum(p[:, np.clip(xs + k, 0, W1 - 1)] for k in range(-R, R + 1))


def warm_costs(h, a, e, blockSize):
    """T3: C'(y) for y in [a, min(a + R, e)) -> int64 [rows, W1, D]"""
    H = h.shape[0]
    R = blockSize // 2
    rows = range(a, min(a + R, e))
    out = np.zeros((len(rows),) + h.shape[1:], np.int64)
    for i, y in enumerate(rows):
        for j in range(-R, R + 1):
            out[i] += h[min(max(y + j, a), H - 1)]
    return out


def aggregate(pix, Cc, P1, P2, blockSize, nstripes=NSTRIPES, floor=True):
    """T3-T5 -> (S uint16 [H, W1, D], the largest block cost read, C' included).  floor=False drops T3: every row reads C."""
    H, W1, D = Cc.shape
    Lh = sgm_hh4_ref.path_costs(Cc, 1, 0, P1, P2) + sgm_hh4_ref.path_costs(Cc, -1, 0, P1, P2)
    h = row_sums(pix, blockSize) if floor else None
    S = np.zeros(Cc.shape, np.int64)
    cmax = int(Cc.max())
    for a, o, e in stripes(H, blockSize, nstripes):
        if o >= e:
            continue
        Cs = Cc[a:e].astype(np.int64)
        if floor and a > 0:
            Cw = warm_costs(h, a, e, blockSize)
            cmax = max(cmax, int(Cw.max()) if Cw.size else 0)
            Cs[:len(Cw)] = Cw
        Ld = sgm_hh4_ref.path_costs(np.minimum(Cs, 65535).astype(np.uint16), 0, 1, P1, P2)
        S[o:e] = np.minimum(np.minimum(Lh[o:e], 32767) + Ld[o - a:], 32767)             # R5, the grouping does not matter
    return S.astype(np.uint16), cmax


def params_of(**kw):
    from oracle import oracle as orc
    kw = dict(kw)
    kw["paths"] = 8                                             # (what the oracle's structure is given; the mode is this file)
    kw["disp12MaxDiff"] = NEVER                                 # T6: accepted and ignored
    return orc.make_sgm_params(**kw)


def sgm_compute(left, right, preFilterCap=0, census=None, nstripes=NSTRIPES, floor=True, **kw):
    """What the device computes under MODE_SGBM_3WAY for a gray or colour pair.  Raises CostOverflow where it refuses the frame."""
    left = np.ascontiguousarray(left, np.uint8); right = np.ascontiguousarray(right, np.uint8)
    assert left.shape == right.shape and left.ndim in (2, 3)
    H, W = left.shape[:2]
    kw.pop("disp12MaxDiff", None); kw.pop("paths", None)
    p = params_of(**kw)
    D, minD = p.numDisparities, p.minDisparity
    W1 = (W + min(minD, 0)) - max(minD + D, 0)
    if W1 <= 0:
        return np.full((H, W), (minD - 1) * 16, np.int16)
    P1 = p.P1 if p.P1 > 0 else 2
    P2 = max(p.P2 if p.P2 > 0 else 5, P1 + 1)
    pix = pixel_costs(left, right, p, preFilterCap, census)
    Cc, _ = block_costs(pix, p.blockSize)
    S, cmax = aggregate(pix, Cc, P1, P2, p.blockSize, nstripes, floor)
    if cmax + P2 > 32767:                                       # T8
        raise CostOverflow("largest block cost %d + P2 %d > 32767" % (cmax, P2))
    return sgm_hh4_ref.finish(S, W, H, p)


def valid_share(disp, minD, D):
    """share of the column domain's pixels that carry a disparity"""
    W = disp.shape[1]
    dom = disp[:, max(minD + D, 0):W + min(minD, 0)]
    return float((dom != (minD - 1) * 16).mean())
