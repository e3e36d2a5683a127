"""numpy restatement of rules X1-X7: reprojectImageTo3D on an x16 disparity map and the point cloud
of the pixels calc_depth keeps.  Elementwise float64 operations in the X2 order (numpy never fuses a multiply with an add),
one division, one rounding to float32; boolean indexing for the cloud.  Test infrastructure: the product never imports it."""
import numpy as np

FIXED16, ROUNDED = 0, 1
POINT = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("r", "u1"), ("g", "u1"), ("b", "u1"), ("a", "u1")])
FLT_EPSILON = float(np.finfo(np.float32).eps)


def disparity(disp, mode):
    """X1: the disparity as float64."""
    d = np.asarray(disp, np.int16).astype(np.float64) / 16.0            # exact
    # rint: half to even.  The reference's rounded map is CV_16S, an integer, so a zero is +0.0: `+ 0.0` turns the -0.0 that
    # rint gives for d in [-0.5, -0.0) into it (the sign of zero can decide between +inf and -inf in X3)
    return np.rint(d) + 0.0 if mode == ROUNDED else d


def reproject(disp, Q, mode=ROUNDED, handle_missing_values=True):
    """X2-X5: int16 H x W -> float32 H x W x 3."""
    q = np.asarray(Q, np.float64).reshape(16)
    d = disparity(disp, mode)
    H, W = d.shape
    x = np.arange(W, dtype=np.float64)[None, :] * np.ones((H, 1))
    y = np.arange(H, dtype=np.float64)[:, None] * np.ones((1, W))
    h = [((q[4 * r] * x + q[4 * r + 1] * y) + q[4 * r + 2] * d) + q[4 * r + 3] for r in range(4)]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        xyz = np.stack([(h[r] / h[3]).astype(np.float32) for r in range(3)], axis=2)
    if handle_missing_values:
        xyz[..., 2][d == d.min()] = np.float32(10000.0)                 # X4
    return xyz


def keep(disp, xyz, min_disparity=0, max_z=1e4, mask=None):
    """X6: the boolean H x W map of the pixels the cloud keeps."""
    z = xyz[..., 2].astype(np.float64)
    with np.errstate(invalid="ignore"):
        k = (np.asarray(disp, np.int32) != (min_disparity - 1) * 16) & (np.abs(z - 10000.0) >= FLT_EPSILON) & (np.abs(z) <= max_z)
    if mask is not None:
        k &= np.asarray(mask) != 0
    return k


def cloud(disp, Q, mode=ROUNDED, handle_missing_values=True, min_disparity=0, max_z=1e4, guide=None, mask=None):
    """X7: the records of the kept pixels in row-major order (all of them; the caller cuts at its capacity)."""
    xyz = reproject(disp, Q, mode, handle_missing_values)
    k = keep(disp, xyz, min_disparity, max_z, mask)
    pts = np.zeros(int(k.sum()), POINT)
    pts["x"], pts["y"], pts["z"] = xyz[..., 0][k], xyz[..., 1][k], xyz[..., 2][k]
    pts["a"] = 255
    if guide is not None:
        g = np.asarray(guide, np.uint8)
        if g.ndim == 2 or g.shape[2] == 1:
            pts["r"] = pts["g"] = pts["b"] = g.reshape(g.shape[:2])[k]
        else:
            pts["r"], pts["g"], pts["b"] = g[..., 0][k], g[..., 1][k], g[..., 2][k]
    return pts
