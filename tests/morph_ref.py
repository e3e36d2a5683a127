"""Plain-numpy reference of the general morphology path (rules M1-M7), written from the rules and
independently of the C code: the three element shapes of cv::getStructuringElement, erosion / dilation as a minimum /
maximum over shifted copies of a neutrally padded frame (any mask, any anchor), and the eight operations with iterations.
tests/test_morph_general_cpu.py pins it against the oracle, the stored goldens and scipy."""
import numpy as np

RECT, CROSS, ELLIPSE = 0, 1, 2
ERODE, DILATE, OPEN, CLOSE, GRADIENT, TOPHAT, BLACKHAT, OPEN_CLOSE = 0, 1, 2, 3, 4, 5, 6, 100
OPS = (ERODE, DILATE, OPEN, CLOSE, GRADIENT, TOPHAT, BLACKHAT, OPEN_CLOSE)


def element(shape, w, h):
    """bool array h x w; the anchor that goes with it is (w // 2, h // 2)."""
    if w == 1 and h == 1:
        shape = RECT
    e = np.zeros((h, w), bool)
    if shape == RECT:
        e[:] = True
    elif shape == CROSS:
        e[h // 2, :] = True
        e[:, w // 2] = True
    elif shape == ELLIPSE:
        r, c = h // 2, w // 2
        for i in range(h):
            dy = i - r
            if abs(dy) > r:
                continue
            dx = int(np.rint(c * np.sqrt((r * r - dy * dy) / float(r * r)))) if r else 0      # cvRound: ties to even
            e[i, max(c - dx, 0):min(c + dx + 1, w)] = True
    else:
        raise ValueError(shape)
    return e


def _extremum(img, el, anchor, dilate):
    el = np.asarray(el) != 0
    kh, kw = el.shape
    ax, ay = (kw // 2, kh // 2) if anchor is None else anchor
    H, W = img.shape
    neutral = 0 if dilate else 255
    pad = np.full((H + kh - 1, W + kw - 1), neutral, np.uint8)       # frame pixel (y, x) at (y + ay, x + ax)
    pad[ay:ay + H, ax:ax + W] = img
    out = np.full((H, W), neutral, np.uint8)
    for i, j in zip(*np.nonzero(el)):                                # member (i, j) samples src(y + i - ay, x + j - ax)
        out = (np.maximum if dilate else np.minimum)(out, pad[i:i + H, j:j + W])
    return out


def erode(img, el, anchor=None, iterations=1):
    for _ in range(iterations):
        img = _extremum(img, el, anchor, False)
    return img


def dilate(img, el, anchor=None, iterations=1):
    for _ in range(iterations):
        img = _extremum(img, el, anchor, True)
    return img


def _diff(a, b):
    return np.clip(a.astype(np.int16) - b.astype(np.int16), 0, 255).astype(np.uint8)


def morphology(img, op, el, anchor=None, iterations=1):
    n = iterations
    e = lambda s: erode(s, el, anchor, n)       # noqa: E731
    d = lambda s: dilate(s, el, anchor, n)      # noqa: E731
    if op == ERODE:
        return e(img)
    if op == DILATE:
        return d(img)
    if op == OPEN:
        return d(e(img))
    if op == CLOSE:
        return e(d(img))
    if op == GRADIENT:
        return _diff(d(img), e(img))
    if op == TOPHAT:
        return _diff(img, d(e(img)))
    if op == BLACKHAT:
        return _diff(e(d(img)), img)
    if op == OPEN_CLOSE:
        return e(d(d(e(img))))
    raise ValueError(op)


def gray_frame(W, H, seed):
    """A low-frequency ramp plus noise, never saturated: the darkest pixels are at the left, the brightest at the right, so
    a window that does not cover the whole frame still gives a result that varies."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    ramp = 32 + 150.0 * xx / max(W - 1, 1) + 24.0 * yy / max(H - 1, 1) + 10 * np.sin(xx / 9.0 + seed) * np.cos(yy / 7.0)
    return np.clip(ramp + rng.integers(-15, 16, (H, W)), 0, 255).astype(np.uint8)


def mask_frame(W, H, seed):
    """Blobs plus salt and pepper, 0 / 255.  The left third is a clean solid block beside a clean empty one, so that an
    erosion or dilation with an element up to about a sixth of the frame leaves both values."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    m = np.zeros((H, W), bool)
    for _ in range(max(2, W * H // 900)):
        cx, cy, r = rng.integers(0, W), rng.integers(0, H), rng.integers(2, 3 + max(W, H) // 4)
        m |= (xx - cx) ** 2 + (yy - cy) ** 2 <= r * r
    m ^= rng.random((H, W)) < 0.04
    m[:, :W // 3] = False
    m[:, :W // 6] = True
    return (m * 255).astype(np.uint8)


def random_element(w, h, seed):
    """Several runs per row, an empty first row and last column where the size allows, never empty altogether."""
    rng = np.random.default_rng(seed)
    e = rng.random((h, w)) < 0.45
    if h > 2:
        e[0, :] = False
    if w > 2:
        e[:, -1] = False
    e[h // 2, 0] = True
    if w > 3:
        e[h // 2, 1], e[h // 2, 2] = False, True                      # two runs in one row at least
    return e
