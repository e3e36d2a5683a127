"""The disparity WLS post-filter (rules W1-W8): the reference the GPU tests compare against.

A NumPy restatement in float64 of what rtdm_wls_* compute: the right matcher's parameters (W1), the filter's parameters
(W2), the discontinuity maps (W3), the confidence (W4), the weight table and weights (W5), the fast global smoother as Thomas
solves vectorised over rows / columns (W6), the combination (W7) and the output (W8).  The weight table is the same float32
table the device uses.  Like the rest of the oracle, parity with cv::ximgproc itself is unpinned.
"""
import math

import numpy as np

LUT_N = 3 * 255 * 255 + 1


def lut(sigma):
    """W5: exp(-sqrt(k) / sigma) in double, rounded to float32, values below FLT_MIN flushed to 0."""
    v = np.exp(-np.sqrt(np.arange(LUT_N, dtype=np.float64)) / sigma).astype(np.float32)
    v[v < np.finfo(np.float32).tiny] = 0
    return v


def _common():
    return dict(lambda_=8000.0, sigma_color=1.5, lrc_thresh=24, num_iter=3, attenuation=0.25, use_confidence=1)


def params_for_bm(blockSize, minDisparity, numDisparities):
    w, m, n = blockSize, minDisparity, numDisparities
    p = _common()
    p.update(depth_discontinuity_radius=int(math.ceil(0.33 * w)), min_disparity=m, num_disparities=n,
             roi_left=max(0, m + n) + w // 2, roi_right=max(0, -m) + w // 2, roi_top=w // 2, roi_bottom=w // 2)
    return p


def params_for_sgm(blockSize, minDisparity, numDisparities):
    w, m, n = blockSize, minDisparity, numDisparities
    p = _common()
    p.update(depth_discontinuity_radius=int(math.ceil(0.5 * w)), min_disparity=m, num_disparities=n,
             roi_left=max(0, m + n), roi_right=max(0, -m), roi_top=0, roi_bottom=0)
    return p


def right_min_disparity(minDisparity, numDisparities):
    return -(minDisparity + numDisparities) + 1


def roi(p, W, H):
    """(x0, x1, y0, y1) of the valid ROI, or None when it is empty."""
    x0, x1, y0, y1 = p["roi_left"], W - p["roi_right"], p["roi_top"], H - p["roi_bottom"]
    return (x0, x1, y0, y1) if x1 > x0 and y1 > y0 else None


def _window(v, valid, r, axis):
    """min / max / count of the valid values in a (2r+1) window along `axis`, clipped to the frame"""
    big = np.iinfo(np.int32).max
    mn = np.where(valid, v, big).astype(np.int64)
    mx = np.where(valid, v, -big).astype(np.int64)
    ct = valid.astype(np.int64)
    L = v.shape[axis]
    omn, omx, oct_ = mn.copy(), mx.copy(), ct.copy()
    for k in range(1, min(r, L - 1) + 1):
        for s in (k, -k):
            sl_dst = [slice(None)] * v.ndim
            sl_src = [slice(None)] * v.ndim
            sl_dst[axis] = slice(max(0, -s), L - max(0, s))
            sl_src[axis] = slice(max(0, s), L - max(0, -s))
            d, sr = tuple(sl_dst), tuple(sl_src)
            omn[d] = np.minimum(omn[d], mn[sr])
            omx[d] = np.maximum(omx[d], mx[sr])
            oct_[d] += ct[sr]
    return omn, omx, oct_


def disc(d, invalid, r, T):
    """W3: 0 where the (2r+1)^2 window holds two or more valid values whose range exceeds T, else 1."""
    d = d.astype(np.int64)
    mn, mx, ct = _window(d, d != invalid, r, 1)
    valid_rows = ct > 0
    big = np.iinfo(np.int32).max
    mn2, _, _ = _window(np.where(valid_rows, mn, big), np.ones_like(valid_rows), r, 0)
    _, mx2, _ = _window(np.where(valid_rows, mx, -big), np.ones_like(valid_rows), r, 0)
    L = ct.shape[0]
    cs = np.concatenate([np.zeros((1,) + ct.shape[1:], np.int64), np.cumsum(ct, axis=0)])
    i = np.arange(L)
    ct2 = cs[np.minimum(i + r + 1, L)] - cs[np.maximum(i - r, 0)]          # valid values in the whole window
    # (a row window without valid values contributes +-big, which the two-value condition below never lets through)
    return np.where((ct2 >= 2) & (mx2 - mn2 > T), 0, 1).astype(np.int64)


def confidence(dL, dR, p):
    """W4: float64 map in {0, 255}, 0 outside the valid ROI."""
    H, W = dL.shape
    invL = (p["min_disparity"] - 1) * 16
    invR = (right_min_disparity(p["min_disparity"], p["num_disparities"]) - 1) * 16
    r, T = p["depth_discontinuity_radius"], p["lrc_thresh"]
    C = np.zeros((H, W))
    box = roi(p, W, H)
    if box is None:
        return C
    dLi = dL.astype(np.int64)
    dRi = dR.astype(np.int64)
    dcL, dcR = disc(dLi, invL, r, T), disc(dRi, invR, r, T)
    x0, x1, y0, y1 = box
    y, x = np.mgrid[y0:y1, x0:x1]
    d = dLi[y0:y1, x0:x1]
    xp = x - np.trunc(d / 16).astype(np.int64)              # C++ truncating division
    inside = (d != invL) & (xp >= 0) & (xp < W)
    xpc = np.clip(xp, 0, W - 1)
    e = dRi[y, xpc]
    ok = inside & (e != invR) & (np.abs(d + e) <= T)
    C[y0:y1, x0:x1] = np.where(ok, 255.0 * dcL[y0:y1, x0:x1] * dcR[y, xpc], 0.0)
    return C


def weights(G, table, box):
    """W5: (wh, wv) float64 over the ROI: wh[y, x] couples (y, x-1) and (y, x), wv[y, x] couples (y-1, x) and (y, x); 0 on the
    ROI's first column / row."""
    x0, x1, y0, y1 = box
    g = G.astype(np.int64)
    if g.ndim == 2:
        g = g[:, :, None]
    g = g[y0:y1, x0:x1]
    h, w = g.shape[:2]
    wh = np.zeros((h, w)); wv = np.zeros((h, w))
    wh[:, 1:] = table[((g[:, 1:] - g[:, :-1]) ** 2).sum(2)]
    wv[1:, :] = table[((g[1:] - g[:-1]) ** 2).sum(2)]
    return wh, wv


def thomas(a, b, c, f):
    """Solve N tridiagonal systems at once: a, b, c (N, L) sub / main / super diagonals, f (N, L, K)."""
    N, L = b.shape
    cp = np.empty((N, L)); dp = np.empty(f.shape)
    cp[:, 0] = c[:, 0] / b[:, 0]
    dp[:, 0] = f[:, 0] / b[:, 0, None]
    for j in range(1, L):
        den = b[:, j] - a[:, j] * cp[:, j - 1]
        cp[:, j] = c[:, j] / den
        dp[:, j] = (f[:, j] - a[:, j, None] * dp[:, j - 1]) / den[:, None]
    u = np.empty(f.shape)
    u[:, L - 1] = dp[:, L - 1]
    for j in range(L - 2, -1, -1):
        u[:, j] = dp[:, j] - cp[:, j, None] * u[:, j + 1]
    return u


def pass_matrices(w, lam):
    """W6 for lines along axis 1: a_j = -lam w(j-1, j), c_j = -lam w(j, j+1), b_j = 1 - a_j - c_j."""
    a = -lam * w
    c = np.zeros_like(w)
    c[:, :-1] = -lam * w[:, 1:]
    return a, 1.0 - a - c, c


def lambdas(p):
    T = p["num_iter"]
    lam = 1.5 * p["lambda_"] * 4.0 ** (T - 1) / (4.0 ** T - 1.0)
    out = []
    for _ in range(T):
        out.append(lam)
        lam *= p["attenuation"]
    return out


def fgs(f, wh, wv, p):
    """W6 on the ROI: f (h, w, K) -> the K smoothed planes."""
    u = f.astype(np.float64)
    for lam in lambdas(p):
        a, b, c = pass_matrices(wh, lam)
        u = thomas(a, b, c, u)
        a, b, c = pass_matrices(wv.T, lam)
        u = thomas(a, b, c, u.transpose(1, 0, 2)).transpose(1, 0, 2)
    return u


def wls_filter(dL, G, p, dR=None):
    """W7 / W8 -> dict(out int16, filtered float64, F1, F2 (float64, NaN outside the ROI), conf float64)."""
    H, W = dL.shape
    inv = (p["min_disparity"] - 1) * 16
    out = np.full((H, W), inv, np.int16)
    filt = np.full((H, W), float(inv))
    F1 = np.full((H, W), np.nan); F2 = np.full((H, W), np.nan)
    conf = confidence(dL, dR, p) if p["use_confidence"] else np.zeros((H, W))
    box = roi(p, W, H)
    if box is None:
        return dict(out=out, filtered=filt, F1=F1, F2=F2, conf=conf)
    x0, x1, y0, y1 = box
    d = dL[y0:y1, x0:x1].astype(np.float64)
    if p["use_confidence"]:
        c = conf[y0:y1, x0:x1]
        f = np.stack([c * d, c], axis=2)
    else:
        f = np.stack([d, np.ones_like(d)], axis=2)
    wh, wv = weights(G, lut(p["sigma_color"]).astype(np.float64), box)
    u = fgs(f, wh, wv, p)
    F1[y0:y1, x0:x1], F2[y0:y1, x0:x1] = u[..., 0], u[..., 1]
    if p["use_confidence"]:
        with np.errstate(divide="ignore", invalid="ignore"):
            v = np.where(u[..., 1] != 0, u[..., 0] / u[..., 1], float(inv))
    else:
        v = u[..., 0]
    filt[y0:y1, x0:x1] = v
    out[y0:y1, x0:x1] = np.clip(np.rint(v), -32768, 32767).astype(np.int16)
    return dict(out=out, filtered=filt, F1=F1, F2=F2, conf=conf)
