"""ROI sets and matcher configurations for the geometry header (csrc/rtdm_bm_geom.h), and make_geom restated in Python integers.

A configuration is (W, H, D, minD, w, disp12MaxDiff, roi2 or None); an ROI is (x, y, w, h) or None ("no ROI1").  lines() is
what tests/bm_geom_host.cpp reads, one case per line."""
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1

CONFIGS = (
    (160, 120, 64, 0, 9, 1, None),
    (97, 65, 16, 0, 9, 1, None),
    (96, 64, 16, 4, 7, 1, None),
    (96, 64, 16, -3, 7, -1, None),
    (120, 80, 16, 0, 7, 1, (10, 5, 100, 70)),
    (300, 80, 80, 0, 21, -1, (-5, -5, 400, 200)),
    (96, 64, 16, -20, 5, 1, None),           # minD + D - 1 < 0: an ROI1 left of the frame reaches columns "no ROI1" does not
    (96, 64, 16, -20, 5, 1, (-30, 0, 200, 64)),
    (40, 30, 64, 0, 5, 1, None),             # lofs >= W: nothing is ever valid
    (934, 404, 64, 0, 9, 1, None),
)


def rois(W, H):
    """[(roi, host_safe)]: host_safe -- 32-bit arithmetic does not overflow on it, so the parent's make_geom is defined there"""
    out = [None,
           (W // 5, H // 5, W // 2, H // 2), (0, 0, W, H), (-100, -100, W + 200, H + 200),        # inside, whole, larger
           (-10, H // 4, W // 2, H // 2), (W // 4, -7, W // 2, H // 2),                            # cut by each edge
           (W - 30, H // 4, 50, H // 2), (W // 4, H - 20, W // 2, 40),
           (-13, -9, W // 2 + 13, H // 2 + 9), (-50, -50, 40, 40), (-50, 3, 45, 40),               # negative origins
           (W // 3, H // 3, 3, H // 3), (W // 3, H // 3, W // 3, 2), (W // 3 + 1, H // 3 + 1, 1, 1),   # narrower than the window
           (5, 5, 0, 10), (5, 5, 10, -1), (5, 5, -7, -7), (0, 0, 0, 0),                            # w or h <= 0
           (W + 10, 2, 20, 20), (3, H + 4, 20, 20),                                                # beyond the far edges
           (17, 11, W // 2 + 1, H // 2 + 1), (23, 12, W // 2, H // 2)]                             # odd / even first rows
    out = [(r, True) for r in out]
    base = (W // 5, H // 5, W // 2, H // 2)
    for i in range(4):
        for v in (INT_MIN, INT_MAX, INT_MIN + 1, INT_MAX - 1, 2 ** 30, -2 ** 30):
            r = list(base); r[i] = v
            out.append((tuple(r), False))
    for r in ((INT_MAX,) * 4, (INT_MIN,) * 4, (INT_MIN, INT_MIN, INT_MAX, INT_MAX), (INT_MAX, INT_MAX, INT_MIN, INT_MIN),
              (1, 1, INT_MAX, INT_MAX), (2 ** 31 - 100, 3, 200, 20), (-2 ** 31, -2 ** 31, 2 ** 31 - 1, 2 ** 31 - 1)):
        out.append((r, False))
    return out


def rect(cfg, roi, envelope=False):
    """make_geom's rectangles in Python integers: (vx0, vx1, vy0, vy1, cx0, cx1, any), saturated to int like the header"""
    W, H, D, minD, w, d12, roi2 = cfg
    r = w // 2
    r1 = [0, 0, W, H]
    r2 = [0, 0, W, H]
    if roi is not None and roi[2] > 0 and roi[3] > 0:
        r1 = list(roi)
    if roi2 is not None and roi2[2] > 0 and roi2[3] > 0:
        r2 = list(roi2)
    lofs, rofs = max(D - 1 + minD, 0), -min(D - 1 + minD, 0)
    width1 = W - rofs - D + 1
    maxD = minD + D - 1
    a0, b0, a1, b1 = r1[0], r1[1], r1[0] + r1[2], r1[1] + r1[3]
    if envelope:
        a0 = b0 = -2 ** 40
        a1 = b1 = 2 ** 40
    xmin = max(a0, r2[0] + maxD) + r
    xmax = min(a1, r2[0] + r2[2] - minD) - r
    ymin = max(b0, r2[1]) + r
    ymax = min(b1, r2[1] + r2[3]) - r
    xmin, xmax = max(xmin, 0), min(xmax, W)
    ymin, ymax = max(ymin, r), min(ymax, H - r)
    reach = D + abs(minD) + 2 if d12 >= 0 else 0
    cx0 = max(lofs, xmin - reach)
    cx1 = min(min(W, lofs + width1), xmax + reach)
    any_ = not (lofs >= W or rofs >= W or width1 < 1) and xmax > xmin and ymax > ymin
    sat = lambda v: max(INT_MIN, min(INT_MAX, v))
    return (sat(xmin), sat(xmax), sat(ymin), sat(ymax), sat(cx0), sat(cx1), int(any_))


def cases():
    """[(cfg, roi, envelope, host_safe)] in the order of lines()"""
    out = []
    for cfg in CONFIGS:
        for roi, safe in rois(cfg[0], cfg[1]):
            out.append((cfg, roi, False, safe))
        out.append((cfg, None, True, False))
    return out


def lines():
    txt = []
    for (W, H, D, minD, w, d12, roi2), roi, env, _ in cases():
        r2 = roi2 or (0, 0, 0, 0)
        r1 = roi or (0, 0, 0, 0)
        txt.append(" ".join(str(int(v)) for v in (W, H, D, minD, w // 2, int(d12 >= 0), *r2, int(roi is not None), *r1, int(env))))
    return "\n".join(txt) + "\n"
