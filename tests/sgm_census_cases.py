"""Inputs and route cases of the census-cost tests (test_sgm_census_cpu.py checks on the CPU that they do what they are built for,
test_gpu_sgm_census.py runs them on the device)."""
import numpy as np

# W, H, D, minD, blockSize, paths, (cw, ch), n, P2 -- and what the case covers
ROUTES = [
    (64, 40, 16, 0, 5, 5, (9, 7), 1, 2400),      # fused
    (97, 49, 32, 0, 3, 8, (5, 5), 2, 2400),      # pitch > W; crosses the 48-row strip
    (70, 9, 16, 0, 1, 4, (3, 3), 1, 2400),       # Rw = 0, "vert"
    (40, 3, 16, 0, 7, 5, (9, 7), 1, 2400),       # H below both windows
    (19, 5, 16, 0, 5, 8, (9, 7), 1, 2400),       # three domain columns
    (273, 8, 16, 0, 5, 5, (7, 7), 1, 2400),      # W1 = 257: one past the fused tile of 256 columns
    (120, 30, 48, 0, 5, 5, (7, 7), 1, 2400),     # D = 48: unfused
    (90, 33, 32, -8, 9, 8, (9, 3), 1, 2400),     # window 9: unfused; minD < 0
    (90, 33, 32, 4, 5, 5, (3, 7), 3, 2400),      # minD > 0, batch, frame stride
    (330, 20, 272, 0, 5, 5, (9, 7), 1, 2400),    # wide-line pass
    (200, 26, 64, 0, 21, 5, (9, 7), 1, 8000),    # checked route: 62 * 441 + 8000 > 32767; the pair is not refused
]
NOISE_CASE = (83, 21, 32, 0, 5, 8, (9, 7), 1, 2400)      # the pure-noise pair: nothing to find, every rule still holds
WINDOWS = [(cw, ch) for cw in (3, 5, 7, 9) for ch in (3, 5, 7)]


def case_id(c):
    W, H, D, minD, bs, paths, (cw, ch), n, P2 = c
    return "%dx%d-D%d-minD%d-bs%d-p%d-c%dx%d-n%d-P2_%d" % (W, H, D, minD, bs, paths, cw, ch, n, P2)


def params(c):
    """the matcher parameters of a case (the speckle filter is off: it would empty the maps of the small cases, which have
    fewer pixels than its window)"""
    W, H, D, minD, bs, paths, census, n, P2 = c
    return dict(numDisparities=D, minDisparity=minD, blockSize=bs, paths=paths, P2=P2, speckleWindowSize=0)


def textured_pair(seed, W, H, shift, top=255, noise=2):
    """A random texture, lightly smoothed, values 0 .. top; the right view is the left one moved by `shift` columns
    (left[x] = right[x - shift]) plus noise of +-`noise` grey levels."""
    rng = np.random.default_rng(seed)
    T = rng.integers(0, top + 1, (H, W + abs(shift))).astype(np.float64)
    T = ((2 * T + np.roll(T, 1, 1) + np.roll(T, 1, 0)) / 4).astype(np.int64)
    if shift >= 0:
        L, R = T[:, :W], T[:, shift:shift + W]
    else:
        L, R = T[:, -shift:-shift + W], T[:, :W]
    R = np.clip(R + rng.integers(-noise, noise + 1, R.shape), 0, top)
    return L.astype(np.uint8).copy(), R.astype(np.uint8).copy()


def noise_pair(seed, W, H):
    rng = np.random.default_rng(seed)
    return tuple(rng.integers(0, 256, (2, H, W)).astype(np.uint8))


def case_frames(i, c):
    """-> (left [n, H, W], right [n, H, W]) of route case i: frame f at disparity minD + 3 + 2 f"""
    W, H, D, minD, bs, paths, census, n, P2 = c
    fr = [textured_pair(9100 + 17 * i + f, W, H, minD + 3 + 2 * f) for f in range(n)]
    return np.stack([f[0] for f in fr]), np.stack([f[1] for f in fr])


def valid_share(disp, c):
    """share of the column domain's pixels that hold a disparity"""
    W, H, D, minD = c[:4]
    x0, x1 = max(minD + D, 0), W + min(minD, 0)
    return float((disp[:, x0:x1] != (minD - 1) * 16).mean())


def lut_pair(seed=9300, W=96, H=30, shift=6):
    """the invariance pair: values 0 .. 120, and the right view through the strictly increasing v -> 2 v + 10"""
    L, R = textured_pair(seed, W, H, shift, top=120)
    return L, R, (2 * R.astype(np.int64) + 10).astype(np.uint8)
