"""The estimator scene of the own-pixel depth tests (rule L7 of DESIGN.md section 4.17): a sensor frame pair with two objects
of ONE colour class -- an L-shaped one, and a square that sits in the free corner of the L's bounding box, 54 pixels from either
bar, so that the default open + close (10x10 ellipse) neither erases nor joins them -- at clearly different disparities.
The texture varies along x only, so the few rows the synthetic pair is off after rectification do not disturb the matcher."""
import numpy as np

import objects_batch_ref as ref

D, BLOCK, MIN_AREA = 32, 7, 40
D_BACK, D_L, D_SQUARE = 3, 9, 21                 # sensor disparities of the background and of the two objects
L_BOX, BAR = (70, 40, 140, 140), 36             # sensor coordinates: the L's box and the width of its two bars
SQUARE = (160, 42, 48, 48)


def shapes(W, H, shift=0):
    yy, xx = np.mgrid[0:H, 0:W]
    x, y, w, h = L_BOX
    x -= shift
    ell = (xx >= x) & (xx < x + w) & (yy >= y) & (yy < y + h) & ((xx < x + BAR) | (yy >= y + h - BAR))
    x, y, w, h = SQUARE
    x -= shift
    return ell, (xx >= x) & (xx < x + w) & (yy >= y) & (yy < y + h)


def columns(seed, W):
    """one gray value per column: a random level every third column, coarse enough to survive the crop's scale of about 0.6"""
    rng = np.random.default_rng(seed)
    t = np.repeat(rng.integers(0, 256, (W + 64) // 3 + 1), 3)[:W + 64].astype(np.float64)
    return (2 * t + np.roll(t, 1) + np.roll(t, -1)) / 4


def pair(c):
    """-> (left, right) sensor RGB frames of the calibration's size"""
    W, H = c["W"], c["H"]
    out = []
    for right in (False, True):
        def tex(seed, d):
            t = columns(seed, W)
            return np.tile(t[np.arange(W) + (d if right else 0)].astype(np.uint8), (H, 1))
        g = tex(41, D_BACK)
        rgb = np.stack([g, g, g], -1)
        ell, square = shapes(W, H, D_L if right else 0)[0], shapes(W, H, D_SQUARE if right else 0)[1]
        for m, seed, d in ((ell, 42, D_L), (square, 43, D_SQUARE)):
            # the object carries its own texture, which moves with it
            t = np.tile(columns(seed, W)[np.arange(W) + (d if right else 0) + 16].astype(np.uint8), (H, 1)).astype(np.int32)
            red = np.stack([120 + t // 2, t // 4, t // 4], -1).astype(np.uint8)
            rgb[m] = red[m]
        out.append(np.ascontiguousarray(rgb))
    return out[0], out[1]


def ranges(oracle):
    return [(oracle.HSV_LOW, oracle.HSV_HIGH)]


def detect(oracle, c, maps, left):
    """objects_batch_ref.detect on the rectified colour crop, with the reference's filter"""
    col = oracle.rectify_rgb(left, maps[0], maps[1], c["roi"])
    return ref.detect(oracle, col, ranges(oracle), None, MIN_AREA, True, oracle.morph_open_close)
