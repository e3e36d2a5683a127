"""numpy restatement of rules C1-C9: stereoRectify from M1 D1 M2 D2 R T and the image size.  Scalar
float64 arithmetic in the written order; np.float32 exactly where a rule says float32 (the corner and grid points, the
undistorted points, the rectangles and their x + w / y + h sums).  Test infrastructure: the product never imports it."""
import math

import numpy as np

ZERO_DISPARITY = 1024
f32 = np.float32


class Unsupported(Exception):
    pass


def rodrigues_to_vec(R):
    """C1, matrix -> rotation vector (closed form)."""
    R = np.asarray(R, np.float64).reshape(3, 3)
    rx, ry, rz = R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]
    s = math.sqrt((rx * rx + ry * ry + rz * rz) * 0.25)
    c = (R[0, 0] + R[1, 1] + R[2, 2] - 1) * 0.5
    c = 1.0 if c > 1.0 else -1.0 if c < -1.0 else c
    theta = math.acos(c)
    if s < 1e-5:
        if c > 0:
            return np.zeros(3)
        raise Unsupported("rotation by pi")
    vth = 1 / (2 * s)
    vth *= theta
    return np.array([rx * vth, ry * vth, rz * vth])


def rodrigues_to_mat(r):
    """C1, rotation vector -> matrix: R = cos(theta) I + (1 - cos(theta)) r r^T + sin(theta) [r]x."""
    x, y, z = (float(v) for v in r)
    theta = math.sqrt(x * x + y * y + z * z)
    if theta < np.finfo(np.float64).eps:
        return np.eye(3)
    c, s = math.cos(theta), math.sin(theta)
    c1 = 1.0 - c
    it = 1.0 / theta
    x, y, z = x * it, y * it, z * it
    rrt = ((x * x, x * y, x * z), (x * y, y * y, y * z), (x * z, y * z, z * z))
    rx = ((0.0, -z, y), (z, 0.0, -x), (-y, x, 0.0))
    return np.array([[c * (1.0 if i == j else 0.0) + c1 * rrt[i][j] + s * rx[i][j] for j in range(3)] for i in range(3)])


def matmul3(A, B):
    return np.array([[A[i][0] * B[0][j] + A[i][1] * B[1][j] + A[i][2] * B[2][j] for j in range(3)] for i in range(3)])


def matvec3(A, v):
    return np.array([A[i][0] * v[0] + A[i][1] * v[1] + A[i][2] * v[2] for i in range(3)])


def undistort_point(u, v, M, D, RR=None):
    """C8: one float32 point -> (float32, float32)."""
    fx, fy, cx, cy = M[0][0], M[1][1], M[0][2], M[1][2]
    k = [float(d) for d in D]
    x = (float(u) - cx) * (1.0 / fx)
    y = (float(v) - cy) * (1.0 / fy)
    x0, y0 = x, y
    for _ in range(5):
        r2 = x * x + y * y
        icdist = (1 + ((k[7] * r2 + k[6]) * r2 + k[5]) * r2) / (1 + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2)
        dx = 2 * k[2] * x * y + k[3] * (r2 + 2 * x * x) + k[8] * r2 + k[9] * r2 * r2
        dy = k[2] * (r2 + 2 * y * y) + 2 * k[3] * x * y + k[10] * r2 + k[11] * r2 * r2
        x = (x0 - dx) * icdist
        y = (y0 - dy) * icdist
    if RR is None:
        RR = np.eye(3)
    xx = RR[0][0] * x + RR[0][1] * y + RR[0][2]
    yy = RR[1][0] * x + RR[1][1] * y + RR[1][2]
    ww = 1.0 / (RR[2][0] * x + RR[2][1] * y + RR[2][2])
    return f32(xx * ww), f32(yy * ww)


def rectangles(M, D, R, P, W, H):
    """C7: inner and outer float32 rectangles (x, y, w, h) of the undistorted 9 x 9 grid."""
    RR = matmul3([P[i][:3] for i in range(3)], R)
    pts = [[undistort_point(f32(x) * f32(W) / f32(8), f32(y) * f32(H) / f32(8), M, D, RR) for x in range(9)] for y in range(9)]
    xs = np.array([[p[0] for p in row] for row in pts], np.float32)
    ys = np.array([[p[1] for p in row] for row in pts], np.float32)
    ix0, ix1, iy0, iy1 = xs[:, 0].max(), xs[:, 8].min(), ys[0, :].max(), ys[8, :].min()
    ox0, ox1, oy0, oy1 = xs.min(), xs.max(), ys.min(), ys.max()
    return ((ix0, iy0, f32(ix1 - ix0), f32(iy1 - iy0)), (ox0, oy0, f32(ox1 - ox0), f32(oy1 - oy0)))


def _sides(rect, cx0, cy0, cx, cy, W, H):
    x, y, w, h = rect
    return (cx / (cx0 - float(x)), cy / (cy0 - float(y)), (W - cx) / (float(f32(x + w)) - cx0), (H - cy) / (float(f32(y + h)) - cy0))


def _roi(rect, cx0, cy0, cx, cy, s, W, H):
    x, y, w, h = (float(v) for v in rect)
    rx, ry = math.ceil((x - cx0) * s + cx), math.ceil((y - cy0) * s + cy)
    rw, rh = math.floor(w * s), math.floor(h * s)
    x0, y0, x1, y1 = max(rx, 0), max(ry, 0), min(rx + rw, W), min(ry + rh, H)
    if x1 <= x0 or y1 <= y0:
        return (0, 0, 0, 0)
    return (x0, y0, x1 - x0, y1 - y0)


def roi_arguments(M1, D1, M2, D2, R, T, W, H, flags, alpha):
    """The eight values that C9 hands to ceil / floor, for the tests' distance-from-an-integer check."""
    return stereo_rectify(M1, D1, M2, D2, R, T, W, H, flags, alpha)["roi_args"]


def stereo_rectify(M1, D1, M2, D2, R, T, W, H, flags=ZERO_DISPARITY, alpha=-1.0):
    M = [np.asarray(M1, np.float64).reshape(3, 3), np.asarray(M2, np.float64).reshape(3, 3)]
    D = []
    for d in (D1, D2):
        d = np.asarray(d, np.float64).reshape(-1)
        D.append(np.concatenate([d, np.zeros(14 - d.size)]))
    R = np.asarray(R, np.float64).reshape(3, 3)
    T = np.asarray(T, np.float64).reshape(3)
    # C1
    om = rodrigues_to_vec(R)
    r_r = rodrigues_to_mat(om * -0.5)
    t = matvec3(r_r, T)
    # C2
    idx = 0 if abs(t[0]) > abs(t[1]) else 1
    c, nt = t[idx], math.sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2])
    uu = [0.0, 0.0, 0.0]
    uu[idx] = 1.0 if c > 0 else -1.0
    ww = np.array([t[1] * uu[2] - t[2] * uu[1], t[2] * uu[0] - t[0] * uu[2], t[0] * uu[1] - t[1] * uu[0]])
    nw = math.sqrt(ww[0] * ww[0] + ww[1] * ww[1] + ww[2] * ww[2])
    if nw > 0.0:
        ww = ww * (math.acos(abs(c) / nt) / nw)
    wR = rodrigues_to_mat(ww)
    R1 = matmul3(wR, r_r.T)
    R2 = matmul3(wR, r_r)
    t = matvec3(R2, T)
    Rk = [R1, R2]
    # C3
    fc_new = float("inf")
    for k in range(2):
        fc = M[k][idx ^ 1][idx ^ 1]
        if D[k][0] < 0:
            fc *= 1 + D[k][0] * (W * W + H * H) / (4 * fc * fc)
        fc_new = min(fc_new, fc)
    # C4
    cc = []
    for k in range(2):
        sx = sy = 0.0
        for i in range(4):
            u, v = f32((i % 2) * (W - 1)), f32((i // 2) * (H - 1))
            px, py = undistort_point(u, v, M[k], D[k])
            X, Y, Z = float(px), float(py), 1.0
            x = Rk[k][0][0] * X + Rk[k][0][1] * Y + Rk[k][0][2] * Z
            y = Rk[k][1][0] * X + Rk[k][1][1] * Y + Rk[k][1][2] * Z
            z = Rk[k][2][0] * X + Rk[k][2][1] * Y + Rk[k][2][2] * Z
            z = 1.0 / z if z else 1.0
            x *= z
            y *= z
            sx += float(f32(x * fc_new))
            sy += float(f32(y * fc_new))
        cc.append([(W - 1) / 2 - sx * 0.25, (H - 1) / 2 - sy * 0.25])
    # C5
    if flags & ZERO_DISPARITY:
        cc[0][0] = cc[1][0] = (cc[0][0] + cc[1][0]) * 0.5
        cc[0][1] = cc[1][1] = (cc[0][1] + cc[1][1]) * 0.5
    elif idx == 0:
        cc[0][1] = cc[1][1] = (cc[0][1] + cc[1][1]) * 0.5
    else:
        cc[0][0] = cc[1][0] = (cc[0][0] + cc[1][0]) * 0.5
    P = [np.zeros((3, 4)), np.zeros((3, 4))]
    for k in range(2):
        P[k][0][0] = P[k][1][1] = fc_new
        P[k][0][2], P[k][1][2], P[k][2][2] = cc[k][0], cc[k][1], 1.0
    P[1][idx][3] = t[idx] * fc_new
    # C6, C7
    alpha = min(alpha, 1.0)
    rects = [rectangles(M[k], D[k], Rk[k], P[k], W, H) for k in range(2)]
    c0 = [(cc[k][0], cc[k][1]) for k in range(2)]
    c1 = [(W * cc[k][0] / W, H * cc[k][1] / H) for k in range(2)]
    s = 1.0
    if alpha >= 0:
        s0 = max(max(_sides(rects[k][0], c0[k][0], c0[k][1], c1[k][0], c1[k][1], W, H)) for k in range(2))
        s1 = min(min(_sides(rects[k][1], c0[k][0], c0[k][1], c1[k][0], c1[k][1], W, H)) for k in range(2))
        s = s0 * (1 - alpha) + s1 * alpha
    fc_new *= s
    for k in range(2):
        P[k][0][0] = P[k][1][1] = fc_new
        P[k][0][2], P[k][1][2] = c1[k]
    P[1][idx][3] = s * P[1][idx][3]
    # C9
    rois, args = [], []
    for k in range(2):
        rois.append(_roi(rects[k][0], c0[k][0], c0[k][1], c1[k][0], c1[k][1], s, W, H))
        x, y, w, h = (float(v) for v in rects[k][0])
        args += [(x - c0[k][0]) * s + c1[k][0], (y - c0[k][1]) * s + c1[k][1], w * s, h * s]
    Q = np.zeros((4, 4))
    Q[0][0] = Q[1][1] = 1.0
    Q[0][3], Q[1][3], Q[2][3] = -c1[0][0], -c1[0][1], fc_new
    Q[3][2] = -1.0 / t[idx]
    Q[3][3] = (c1[0][idx] - c1[1][idx]) / t[idx]
    return {"R1": R1, "R2": R2, "P1": P[0], "P2": P[1], "Q": Q, "ROI1": rois[0], "ROI2": rois[1], "roi_args": args, "idx": idx}


def rect_map(M, D, R, P, W, H, accumulate=True):
    """initUndistortRectifyMap(..., CV_16SC2) as orc_init_undistort_rectify_map computes it -> (map1 HxWx2 int16, map2 HxW
    uint16).  accumulate=True is the rule (the ray is summed along the row, one rounding per column); False computes every
    ray directly as x0 + j * ir[0], which is NOT the rule and exists so that a test can tell the two apart."""
    M = np.asarray(M, np.float64).reshape(3, 3)
    d = np.zeros(14)
    dd = np.asarray(D, np.float64).reshape(-1)
    d[:dd.size] = dd
    P = np.asarray(P, np.float64).reshape(3, 4)
    a = matmul3(P[:, :3], np.asarray(R, np.float64).reshape(3, 3)).reshape(9)
    c0, c1, c2 = a[4] * a[8] - a[5] * a[7], a[5] * a[6] - a[3] * a[8], a[3] * a[7] - a[4] * a[6]
    det = a[0] * c0 + a[1] * c1 + a[2] * c2
    i_d = 1.0 / det
    ir = [c0 * i_d, (a[2] * a[7] - a[1] * a[8]) * i_d, (a[1] * a[5] - a[2] * a[4]) * i_d,
          c1 * i_d, (a[0] * a[8] - a[2] * a[6]) * i_d, (a[2] * a[3] - a[0] * a[5]) * i_d,
          c2 * i_d, (a[1] * a[6] - a[0] * a[7]) * i_d, (a[0] * a[4] - a[1] * a[3]) * i_d]
    i = np.arange(H, dtype=np.float64)[:, None]
    ray = []
    for k in range(3):
        start = i * ir[3 * k + 1] + ir[3 * k + 2]
        if accumulate:
            steps = np.full((H, W), ir[3 * k])
            steps[:, :1] = start
            ray.append(np.cumsum(steps, axis=1))                       # sequential: element j = j additions
        else:
            ray.append(start + np.arange(W, dtype=np.float64)[None, :] * ir[3 * k])
    k1, k2, p1, p2, k3, k4, k5, k6, s1, s2, s3, s4 = d[:12]
    w = 1.0 / ray[2]
    x, y = ray[0] * w, ray[1] * w
    x2, y2 = x * x, y * y
    r2, _2xy = x2 + y2, 2 * x * y
    kr = (1 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1 + ((k6 * r2 + k5) * r2 + k4) * r2)
    xd = x * kr + p1 * _2xy + p2 * (r2 + 2 * x2) + s1 * r2 + s2 * r2 * r2
    yd = y * kr + p1 * (r2 + 2 * y2) + p2 * _2xy + s3 * r2 + s4 * r2 * r2
    u, v = M[0, 0] * xd + M[0, 2], M[1, 1] * yd + M[1, 2]
    iu = np.clip(np.rint(u * 32.0), -2147483648.0, 2147483647.0).astype(np.int64)
    iv = np.clip(np.rint(v * 32.0), -2147483648.0, 2147483647.0).astype(np.int64)
    map1 = np.stack([iu >> 5, iv >> 5], -1).astype(np.int16)
    map2 = ((iv & 31) * 32 + (iu & 31)).astype(np.uint16)
    return map1, map2


def check_rectification(got, want, where):
    """the issue's tolerances; want: dict with R1 R2 P1 P2 Q (arrays) and ROI1 ROI2"""
    assert tuple(got["ROI1"]) == tuple(want["ROI1"]) and tuple(got["ROI2"]) == tuple(want["ROI2"]), where
    for k in ("R1", "R2"):
        g, w = np.asarray(got[k]).reshape(-1), np.asarray(want[k], np.float64).reshape(-1)
        assert np.abs(g - w).max() <= 1e-12, (where, k, np.abs(g - w).max())
    for k in ("P1", "P2", "Q"):
        g, w = np.asarray(got[k]).reshape(-1), np.asarray(want[k], np.float64).reshape(-1)
        zero = w == 0
        assert np.all(g[zero] == 0), (where, k)
        rel = np.abs(g[~zero] - w[~zero]) / np.abs(w[~zero])
        assert rel.max() <= 1e-12, (where, k, rel.max())


def tie_calibration():
    """A camera whose exact map coordinates are all ties: u = j - 1/64, v = i - 1/64, so rint(u * 32) is decided by the last
    bits of the accumulated ray.  On the recorded calibrations a directly computed ray happens to give the same maps."""
    f = 300.3
    M = np.array([[f, 0, 160.0], [0, f, 120.0], [0, 0, 1.0]])
    P = np.array([[f, 0, 160 + 1 / 64, 0], [0, f, 120 + 1 / 64, 0], [0, 0, 1.0, 0]])
    return M, np.zeros(14), np.eye(3), P
