"""numpy restatement of rules G1-G8: the per-object measurements of rtdm_objects_measure_device on top
of xyz_ref.reproject -- boolean indexing for the kept pixels, np.sort on the keys for the quantiles, math.fsum for the sums,
cc_labels_ref.clipped for the boxes.  Test infrastructure: the product never imports it."""
import math

import numpy as np

import cc_labels_ref as lr
import xyz_ref as xr

MEASURE = np.dtype([("npix", "<i4"), ("nplane", "<i4"), ("zq", "<f4", (8,)), ("lo", "<f4", (3,)), ("hi", "<f4", (3,)), ("mean", "<f8", (3,))])
ALL_PERMILLE = (0, 500, 1000, 250, 250, 999, 1, 750)


def keys(v):
    """G5: float32 -> uint32 whose unsigned order is the order of the values, -0.0 below +0.0"""
    u = np.ascontiguousarray(v, np.float32).view(np.uint32)
    return np.where(u >> 31 != 0, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def unkeys(k):
    k = np.ascontiguousarray(k, np.uint32)
    return np.where(k >> 31 != 0, k ^ np.uint32(0x80000000), ~k).astype(np.uint32).view(np.float32)


def kept_map(xyz, max_z):
    """G4 without the plane: H x W bool"""
    z = xyz[..., 2].astype(np.float64)
    with np.errstate(invalid="ignore"):
        return (np.abs(z - 10000.0) >= xr.FLT_EPSILON) & (np.abs(z) <= max_z)


def stored_count(counts, capacity):
    return min(int(np.maximum(np.asarray(counts, np.int64), 0).sum()), capacity)


def measure_with_bound(disp, Q, planes, objects, counts, capacity, labels, mode=xr.ROUNDED, max_z=1e4, permille=ALL_PERMILLE, xyz=None):
    """One frame: int16 H x W map, K planes (uint8 masks, or int32 labels with labels=True), the frame's object list
    [(x, y, w, h, cls)] (at least the stored ones) and class counts -> (MEASURE records of the stored objects, the tolerance of
    their means [stored, 3]).
    The tolerance of mean[j] is npix * 2^-52 * sum |v_j| / npix: twice what any order of a double sum of npix terms can differ
    from the exact sum (npix * 2^-53 * sum |v_j|), divided by npix -- once for the sum, once for the division."""
    H, W = np.asarray(disp).shape
    K = len(planes)
    if xyz is None:
        xyz = xr.reproject(disp, Q, mode, True)                              # G3: X4 always on
    keep = kept_map(xyz, max_z)
    stored = stored_count(counts, capacity)
    out = np.zeros(stored, MEASURE)
    bound = np.zeros((stored, 3))
    for i in range(stored):
        o = objects[i]
        box = lr.clipped(o, W, H)
        if box is None or not 0 <= o[4] < K:
            continue                                                         # G8
        x0, y0, w, h = box
        win = (slice(y0, y0 + h), slice(x0, x0 + w))
        plane = np.asarray(planes[o[4]])[win]
        passed = (plane == i + 1) if labels else (plane != 0)                # G2
        out[i]["nplane"] = int(passed.sum())
        k = passed & keep[win]
        n = int(k.sum())
        out[i]["npix"] = n
        if n == 0:
            continue
        pts = xyz[win][k]                                                    # n x 3 float32
        zk = np.sort(keys(pts[:, 2]))
        out[i]["zq"][:len(permille)] = unkeys(zk[[((n - 1) * int(p)) // 1000 for p in permille]])
        kj = keys(pts)
        out[i]["lo"], out[i]["hi"] = unkeys(kj.min(axis=0)), unkeys(kj.max(axis=0))
        wide = pts.astype(np.float64)
        out[i]["mean"] = [math.fsum(wide[:, j].tolist()) / n for j in range(3)]
        bound[i] = n * 2.0 ** -52 * np.abs(wide).sum(axis=0) / n
    return out, bound


def measure_frame(*a, **kw):
    return measure_with_bound(*a, **kw)[0]


def same_exact(got, want):
    """every field but the means, bytewise -> the first differing (index, field) or None"""
    for name in ("npix", "nplane", "zq", "lo", "hi"):
        a, b = np.ascontiguousarray(got[name]), np.ascontiguousarray(want[name])
        if a.tobytes() != b.tobytes():
            rows = np.nonzero((a.reshape(len(a), -1).view(np.uint32) != b.reshape(len(b), -1).view(np.uint32)).any(axis=1))[0]
            return int(rows[0]), name
    return None
