"""Deterministic stereo pairs that ATTAIN the arithmetic bounds of the StereoBM search stage, where natural pairs
(synth.make_pair) stay far below them.  Pure numpy, seeded, no device.

    make(family, seed, W, H, D, minD=0, w=9) -> (L, R)     uint8 [H, W]
    make_n(family, seed, n, W, H, D, minD=0, w=9)          uint8 [n, H, W]: frame i is make(family, seed + i, ...)

Conventions: disparity d means L[y, x] == R[y, x - d]; the search looks at d in [minD, minD + D - 1] and walks the REVERSED
index i = minD + D - 1 - d upwards, so the first minimum is the largest disparity.  The x-Sobel prefilter of a row-constant
image is clamp(4 (I[x+1] - I[x-1]), -cap, cap) + cap: a step of 8 grey levels or more saturates at every cap <= 31, one of 16
at every cap <= 63, so the families below prefilter to the same bytes {0, cap, 2 cap} whatever the cap.

Families (tests/test_hostile_pairs_cpu.py asserts what each one claims):
  worst          period 4, [0, 255, 255, 0], against itself shifted by 2 + seed % 4 columns: every prefiltered byte is 0 or
                 2 cap, and every full window has SAD 2 cap w w -- the most a window can hold -- at the disparities congruent
                 to seed mod 4, 0 at those two away, about half in between.  The prefix sums of every kernel grow as fast as they can.
  worst_noise    column blocks of random width 32 .. 96, alternately `worst` and uint8 noise whose copy in the right view is
                 shifted by a random in-range disparity per block: rows run at the bound next to real, unique minima.
  ties           L == R, row-constant periodic, column blocks of periods 3, 4, 5, 8, 16, 32 (each at least D + 3 w columns wide;
                 one period per seed where the frame has no room for two blocks): the minima tie a period apart.
  plateau_noise  noise whose right view is displaced per band of rows, plus constant blocks in both views (zero texture, every
                 SAD inside them ties) -- the content tests/test_gpu_ring_pair.py was written on.
  edges          noise in bands of rows; the right view is shifted by minD, minD + D - 1, minD - 1, minD + D, minD + 1 and
                 minD + D - 2 in turn: the two ends of the range, one step outside either end, one step inside.
  bars           a constant frame with sparse two-column bar segments; the right view is a shifted copy with some of them
                 removed.  Window and texture sums are small multiples of cap: the thresholds are hit exactly.
  steps          noise whose disparity rises by two every w / 2 + 4 columns (and falls back to the low end of the range at its
                 top): at every step two columns of the left view are hidden behind the nearer surface, so two left pixels
                 two disparities apart claim one right pixel -- what disp12MaxDiff 1 | 2 decides.  (Of the other six families
                 only `bars` makes that boundary live, and only on the D = 272 route.)
"""
import numpy as np

FAMILIES = ("worst", "worst_noise", "ties", "plateau_noise", "edges", "bars", "steps")
P4 = np.array([0, 255, 255, 0], np.uint8)
PERIODS = (3, 4, 5, 8, 16, 32)
EDGE_STEPS = ("minD", "maxD", "minD-1", "maxD+1", "minD+1", "maxD-1")


def worst_shift(seed):
    """The disparities at which `worst` (and the worst blocks of worst_noise) holds the maximal SAD are those congruent to
    this modulo 4; the SAD is 0 at the ones two away."""
    return int(seed) % 4


def _worst_rows(seed, W):
    x = np.arange(W)
    phase = (int(seed) // 4) % 4
    return P4[(x + phase) % 4], P4[(x + phase + 2 + worst_shift(seed)) % 4]


def worst(seed, W, H, D, minD=0, w=9):
    l, r = _worst_rows(seed, W)
    return np.tile(l, (H, 1)), np.tile(r, (H, 1))


def worst_noise_blocks(seed, W, D, minD=0):
    """[(x0, x1, kind, d)]: the column blocks of the left view; kind 'worst' or 'noise' (d = the block's disparity)."""
    rng = np.random.default_rng([int(seed), 11])
    out, x, k = [], 0, int(seed) & 1
    while x < W:
        bw = int(rng.integers(32, 97))
        x1 = W if W - (x + bw) < 32 else x + bw
        d = int(rng.integers(minD, minD + D))
        out.append((x, x1, "noise" if k & 1 else "worst", d))
        x, k = x1, k + 1
    return out


def worst_noise(seed, W, H, D, minD=0, w=9):
    L, R = worst(seed, W, H, D, minD, w)
    rng = np.random.default_rng([int(seed), 12])
    noise = rng.integers(0, 256, (H, W), dtype=np.uint8)
    for x0, x1, kind, d in worst_noise_blocks(seed, W, D, minD):
        if kind != "noise":
            continue
        L[:, x0:x1] = noise[:, x0:x1]
        a, b = max(x0 - d, 0), min(x1 - d, W)              # R[x - d] = L[x]
        if b > a:
            R[:, a:b] = noise[:, a + d:b + d]
    return L, R


def _periodic_row(rng, p, W):
    """A row of period p whose prefiltered bytes have no shorter period at any cap: steps of 16 grey levels or more between
    the neighbours of every column, or none."""
    while True:
        v = rng.integers(1, 14, p) * 16
        g = np.sign(np.roll(v, -1) - np.roll(v, 1))
        if g.any() and all(not np.array_equal(g, np.roll(g, s)) for s in range(1, p)):
            return v[np.arange(W) % p].astype(np.uint8)


def ties_blocks(seed, W, D, w=9):
    """[(x0, x1, period)]: the column blocks; their order rotates with the seed."""
    nb = max(1, min(len(PERIODS), W // (D + 3 * w)))
    edges = [W * k // nb for k in range(nb + 1)]
    return [(edges[k], edges[k + 1], PERIODS[(int(seed) + k) % len(PERIODS)]) for k in range(nb)]


def ties(seed, W, H, D, minD=0, w=9):
    rng = np.random.default_rng([int(seed), 13])
    row = np.empty(W, np.uint8)
    for x0, x1, p in ties_blocks(seed, W, D, w):
        row[x0:x1] = _periodic_row(rng, p, x1 - x0)
    # (the per-row offset of the known-answer test on ties: values stay below 256, so the x-Sobel response is that of the row)
    L = (np.tile(row, (H, 1)) + (np.arange(H)[:, None] % 3) * 7).astype(np.uint8)
    return L, L.copy()


def noise_bands(seed, W, H, D, n=1, band=5):
    """[n, H, W] noise; the right view is the left one displaced by a few columns per band of rows, plus a little noise of
    its own."""
    rng = np.random.default_rng(seed)
    L = rng.integers(0, 256, (n, H, W + D), dtype=np.uint8)
    R = np.empty((n, H, W), np.uint8)
    for y in range(H):
        d = 3 + (y // band * 7) % (D - 6)
        R[:, y] = L[:, y, d:d + W]
    R ^= (rng.random((n, H, W)) < 0.05).astype(np.uint8) * 8
    return np.ascontiguousarray(L[:, :, D:]), R


def plateau_noise_n(seed, W, H, D, n=1, band=5):
    """noise_bands with constant blocks in both views: zero texture, and every SAD inside them ties (the FIRST minimum has to
    win).  The n frames share the blocks' places."""
    L, R = noise_bands(seed, W, H, D, n, band)
    rng = np.random.default_rng(seed + 1)
    for img in (L, R):
        for _ in range(3 + W * H // 1500):
            x, y = int(rng.integers(0, W)), int(rng.integers(0, H))
            img[:, y:y + int(rng.integers(2, 24)), x:x + int(rng.integers(3, 90))] = int(rng.integers(0, 256))
    return L, R


def plateau_noise(seed, W, H, D, minD=0, w=9):
    # noise_bands displaces the right view to the RIGHT (it was written for the right matcher's geometry, views swapped and
    # minDisparity <= 1 - D); with the views swapped here its disparities 4 .. D - 3 lie inside [minD, minD + D - 1]
    L, R = plateau_noise_n(int(seed), W, H, D, 1, 2 * w)     # bands two windows high
    return R[0], L[0]


def edge_shifts(D, minD=0):
    return dict(zip(EDGE_STEPS, (minD, minD + D - 1, minD - 1, minD + D, minD + 1, minD + D - 2)))


def edges_bands(seed, H, D, minD=0, w=9):
    """[(y0, y1, step name, d)]: bands of 2 w rows (two bands of H / 2 rows where 4 w rows do not fit); the last band takes the
    rows that are left.  The two ends of the range come first, in an order that alternates with the seed."""
    hb = 2 * w if H >= 4 * w else max(1, H // 2)
    nb = max(1, H // hb)
    sh = edge_shifts(D, minD)
    order = list(EDGE_STEPS)
    if int(seed) & 1:
        order[0], order[1] = order[1], order[0]
    return [(k * hb, H if k == nb - 1 else (k + 1) * hb, order[k % 6], sh[order[k % 6]]) for k in range(nb)]


def edges(seed, W, H, D, minD=0, w=9):
    rng = np.random.default_rng([int(seed), 14])
    P = D + abs(minD) + 2
    base = rng.integers(0, 256, (H, W + 2 * P), dtype=np.uint8)
    L = np.ascontiguousarray(base[:, P:P + W])
    R = np.empty((H, W), np.uint8)
    for y0, y1, _, d in edges_bands(seed, H, D, minD, w):
        R[y0:y1] = base[y0:y1, P + d:P + d + W]            # R[x] = L[x + d]
    return L, R


def bars(seed, W, H, D, minD=0, w=9):
    rng = np.random.default_rng([int(seed), 15])
    d = minD + (D - 1) // 2 + int(rng.integers(-2, 3))      # the copy's shift: mid-range
    P = D + abs(minD) + 8
    base = np.full((H, W + 2 * P), 128, np.uint8)
    Rb = base.copy()
    for _ in range(max(4, (W + 2 * P) * H // (2 * w * w))):   # one segment per two windows' area
        x = int(rng.integers(1, W + 2 * P - 3))
        y0 = int(rng.integers(-H // 4, H))
        y1 = y0 + int(rng.integers(2, max(3, H // 2)))
        v = int(rng.choice([0, 64, 192, 255]))
        base[max(y0, 0):y1, x:x + 2] = v
        if rng.random() > 0.3:                              # three bars in ten are missing in the right view
            Rb[max(y0, 0):y1, x:x + 2] = v
    L = np.ascontiguousarray(base[:, P:P + W])
    R = np.ascontiguousarray(Rb[:, P + d:P + d + W])        # R[x] = L[x + d]
    return L, R


def steps(seed, W, H, D, minD=0, w=9):
    rng = np.random.default_rng([int(seed), 16])
    L = rng.integers(0, 256, (H, W), dtype=np.uint8)
    R = rng.integers(0, 256, (H, W), dtype=np.uint8)
    lo, hi, sp = minD + 2, minD + D - 3, w // 2 + 4
    d = lo + int(rng.integers(0, max(1, (hi - lo) // 2)))
    for x in range(W):                                      # left to right: the nearer surface overwrites the farther one
        if x and x % sp == 0:
            d = d + 2 if d + 2 <= hi else lo
        if 0 <= x - d < W:
            R[:, x - d] = L[:, x]
    return L, R


_MAKERS = dict(steps=steps, worst=worst, worst_noise=worst_noise, ties=ties, plateau_noise=plateau_noise, edges=edges, bars=bars)


def make(family, seed, W, H, D, minD=0, w=9):
    L, R = _MAKERS[family](int(seed), int(W), int(H), int(D), int(minD), int(w))
    L, R = np.ascontiguousarray(L, np.uint8), np.ascontiguousarray(R, np.uint8)
    assert L.shape == R.shape == (H, W)
    return L, R


def make_n(family, seed, n, W, H, D, minD=0, w=9):
    pairs = [make(family, int(seed) + i, W, H, D, minD, w) for i in range(n)]
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
