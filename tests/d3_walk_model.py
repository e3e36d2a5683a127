"""The walk of an object's box as rule D3 states it, in plain Python: the model whose bits
tests/test_gpu_depth_objects.py and tests/test_gpu_measure.py hold the two band kernels to.

Per band of 16 rows 64 lane accumulators; lane l of a box of width cw owns column l & (lw - 1) and row l // lw of every group
of 64 // lw rows, lw = cw rounded up to a power of two, at most 64; a lane adds its pixels one after the other in float64,
rows ascending and inside a row columns ascending; the lanes fold as v[:32] + v[32:], v[:16] + v[16:], ... down to one
value; the bands add up in ascending order.  Every addition is a single float64 addition: nothing here calls a library sum.

The scene is the smallest on which that order can go wrong: box widths around the powers of two and the wave, heights around
the band, some boxes against or over the right and bottom frame edges, and four boxes as high as the frame (three bands each).
Q has the rows 2 and 3 [0, 0, 0, f] and [0, 0, 1, c] with c = -1000 + 2^-30: with integer d the one product that is not zero is
exact and h_3 = (d - 1000) + 2^-30 is exact too (41 bits), so fused and unfused evaluation give the same Z.

The values are chosen so that the ORDER of the additions shows in the bits.  h_3 is 2^-30 where d = 1000 (TOP of the pixels) and
at least 1 - 2^-30 in magnitude elsewhere, of either sign.  So Z is 9437 at a few pixels -- a partial sum that holds one of
them has its last bit at 2^-39 or above -- and between 2^-17 and 2^-27 in magnitude at the others, with float bits down to
2^-51; X = (x - 70) / h_3 and Y = (y - 20) / h_3 run from 2^36 down to 2^-10 likewise.  A sum over a box spans 64 bits and more
where a double holds 53: every addition of a small term to a partial sum that holds a large one rounds a dozen bits away, and
which additions those are depends on the order.  (Before, with Z = 100 / (d / 8 + 0.5), every sum of the scene was exact and any
order gave the same bits.)  What no choice of values in this form of Q can give is cancellation among the large terms -- a
linear h_3 comes close to zero from one side only --, so the rounding left in a sum is about a unit of its last place: an
order that differs in many additions (row-major) changes about half of the boxes, another fold of the lanes a quarter, and the
two additions of three bands in the other order one box in four of those that have three bands (rnd(u) + rnd(v) differs from
rnd(u + v) for a quarter of the pairs of fractions).  `order_matters` counts it on the CPU and
tests/test_d3_walk_model_cpu.py asserts it for the seed in use: each of these orders changes the bits of every one of the four
sums in several boxes, in mask and in label form, so a kernel that adds in one of them fails the GPU tests.  Test infrastructure:
the product never imports it."""
import itertools

import numpy as np

import cc_labels_ref as lr
import measure_ref as mr
import xyz_ref as xr

BAND = 16
W, H, CAP = 140, 40, 40                                     # 39 boxes: the last slot stays empty
WIDTHS, HEIGHTS = (1, 2, 3, 33, 64, 65, 130), (1, 15, 16, 17, 33)
FILTERED = -16
TALL = ((40, 3), (50, 33), (70, 65), (0, W))                   # (x, width) of four more boxes as high as the frame
TOP = 0.02                                                  # share of the pixels with d = 1000
F, K2, C0 = 0.009 * 2.0 ** -10, 1.0, -1000.0 + 2.0 ** -30   # Z = F / (K2 * d + C0): 9437.2 where d = 1000, else |Z| <= 8.8e-6
Q = np.array([[1, 0, 0, -W / 2], [0, 1, 0, -H / 2], [0, 0, 0, F], [0, 0, K2, C0]], np.float64)


def boxes():
    """every width x every height, in turn at the origin, inside, against the right and bottom edges, and over them; then TALL"""
    out = []
    for j, (w, h) in enumerate(itertools.product(WIDTHS, HEIGHTS)):
        x, y = ((0, 0), (min(5, W - w), min(3, H - h)), (W - w, H - h), (W - w + min(3, w - 1), H - h + min(2, h - 1)))[j % 4]
        out.append((x, y, w, h, 0))
    return out + [(x, 0, w, H, 0) for x, w in TALL]           # three bands each, of 16, 16 and 8 rows


def scene(seed=11):
    """-> (disp int16 H x W: integers x 16 (see the module's docstring) with a share of FILTERED, mask uint8 1 x H x W with about a quarter zeros, labels
    int32 1 x H x W in which object i owns about 0.6 of the pixels of its box that no narrower box took, the boxes)"""
    rng = np.random.default_rng(seed)
    d = rng.integers(2, 2048, (H, W))
    near = rng.random((H, W))
    d = np.where(near < 0.4, rng.integers(985, 1016, (H, W)), d)        # h_3 of either sign, |Z| up to f
    d = np.where(near < TOP, 1000, d)                                   # h_3 = 2^-30
    disp = (d * 16).astype(np.int16)
    disp[rng.random((H, W)) < 0.15] = FILTERED
    mask = rng.choice(np.array([0, 255, 1, 128], np.uint8), (1, H, W))
    bx = boxes()
    labels = np.zeros((1, H, W), np.int32)
    for i in reversed(range(len(bx))):                       # the wide boxes first, so the narrow ones keep theirs
        x0, y0, w, h = lr.clipped(bx[i], W, H)
        win = labels[0, y0:y0 + h, x0:x0 + w]
        win[rng.random((h, w)) < 0.6] = i + 1
    return disp, mask, labels, bx


def passed(plane, i, labels):
    return (plane == i + 1) if labels else (plane != 0)


def depth_z(disp):
    """calc_depth's pixel rule (D2) on this module's Q -> (Z float32 H x W, the pixels that count)"""
    d = xr.disparity(disp, xr.ROUNDED)
    z = (F / (K2 * d + C0)).astype(np.float32)                           # the product and the sum are exact
    z[d == d.min()] = np.float32(10000.0)
    zd = z.astype(np.float64)
    return z, ~((np.abs(zd - 10000.0) < xr.FLT_EPSILON) | (np.abs(zd) > 10000.0))


ORDERS = ("d3", "row_major", "fold_neighbours", "bands_descending")


def walk(box, keep, values, order="d3"):
    """D3 over the clipped box (x0, y0, w, h): keep H x W bool, values a list of H x W float64 -> ([one sum per value], count).
    order: "d3", or one of the orders a wrong kernel might add in -- "row_major" (one accumulator, rows then columns),
    "fold_neighbours" (the lanes fold as v[0::2] + v[1::2], ...), "bands_descending" (the last band first)."""
    x0, y0, cw, ch = box
    x1 = x0 + cw
    lw = 1
    while lw < cw and lw < 64:
        lw <<= 1
    rstep = 64 // lw
    keep, values = keep.tolist(), [v.tolist() for v in values]
    total, n = [0.0] * len(values), 0
    if order == "row_major":
        for y in range(y0, y0 + ch):
            for x in range(x0, x1):
                if keep[y][x]:
                    n += 1
                    total = [t + v[y][x] for t, v in zip(total, values)]
        return total, n
    starts = list(range(0, ch, BAND))
    for r0 in (reversed(starts) if order == "bands_descending" else starts):
        r1 = min(r0 + BAND, ch)
        acc = [[0.0] * 64 for _ in values]
        for lane in range(64):
            col, rof = lane & (lw - 1), lane // lw
            for r in range(r0 + rof, r1, rstep):
                y = y0 + r
                for x in range(x0 + col, x1, lw):
                    if keep[y][x]:
                        n += 1
                        for j, v in enumerate(values):
                            acc[j][lane] = acc[j][lane] + v[y][x]
        for j in range(len(values)):
            v = np.array(acc[j], np.float64)
            for half in (32, 16, 8, 4, 2, 1):
                v = v[0::2] + v[1::2] if order == "fold_neighbours" else v[:half] + v[half:2 * half]
            total[j] = total[j] + float(v[0])
    return total, n


def depth_model(disp, plane, bx, labels, unit=25.0, order="d3"):
    """rtdm_depth_objects_device on one frame and one class -> (mean float64 [len(bx)], npix int32 [len(bx)])"""
    z, counts = depth_z(disp)
    mean, npix = np.zeros(len(bx)), np.zeros(len(bx), np.int32)
    for i, b in enumerate(bx):
        (s,), c = walk(lr.clipped(b, W, H), counts & passed(plane, i, labels), [z.astype(np.float64)], order)
        npix[i] = c
        mean[i] = (s / c) * unit / 10.0 if c > 0 else 0.0
    return mean, npix


def measure_model(disp, plane, bx, labels, mode, order="d3"):
    """rtdm_objects_measure_device on one frame and one class, without the quantiles -> MEASURE records [len(bx)]"""
    xyz = xr.reproject(disp, Q, mode, True)
    keep = mr.kept_map(xyz, 1e4)
    wide = [xyz[..., j].astype(np.float64) for j in range(3)]
    out = np.zeros(len(bx), mr.MEASURE)
    for i, b in enumerate(bx):
        x0, y0, w, h = lr.clipped(b, W, H)
        win = (slice(y0, y0 + h), slice(x0, x0 + w))
        own = passed(plane, i, labels)
        out[i]["nplane"] = int(np.count_nonzero(own[win]))
        s, c = walk((x0, y0, w, h), own & keep, wide, order)
        out[i]["npix"] = c
        if c:
            kj = mr.keys(xyz[win][(own & keep)[win]])
            out[i]["lo"], out[i]["hi"] = mr.unkeys(kj.min(axis=0)), mr.unkeys(kj.max(axis=0))
            out[i]["mean"] = [s[j] / c for j in range(3)]
    return out


def order_matters(labels, mode=xr.FIXED16):
    """For every other order of ORDERS: in how many boxes of the scene do the bits of the depth mean, and of each of the three
    measured means, differ from D3's?  -> {order: (depth, [X, Y, Z])}"""
    disp, mask, planes, bx = scene()
    plane = (planes if labels else mask)[0]
    d0, m0 = depth_model(disp, plane, bx, labels)[0], measure_model(disp, plane, bx, labels, mode)["mean"]
    out = {}
    for order in ORDERS[1:]:
        d1, m1 = depth_model(disp, plane, bx, labels, order=order)[0], measure_model(disp, plane, bx, labels, mode, order)["mean"]
        out[order] = (int((d1.view(np.uint64) != d0.view(np.uint64)).sum()),
                      [int((np.ascontiguousarray(m1[:, j]).view(np.uint64) != np.ascontiguousarray(m0[:, j]).view(np.uint64)).sum()) for j in range(3)])
    return out
