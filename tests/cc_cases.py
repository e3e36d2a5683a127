"""Hostile masks for the component labelling behind the object detection (k_cc_rows / k_cc_merge / k_cc_bbox /
k_cc_collect), shared by tests/test_objects_cases_cpu.py (oracle against scipy, no device) and
tests/test_gpu_objects_raw.py (kernels against the oracle), and the RGB frames that pin the HSV conversion per pixel.

Pure numpy, seeded.  CASES is a list of (name, mask uint8 HxW with values 0 / 255).  What the masks have that a mask
behind an open + close never has: one-pixel lines, contacts through corners only, rings one pixel apart, thousands of
one-pixel components, background that reaches the frame through a one-pixel gap, runs lying on the frame.  Every pattern
that is not symmetric appears mirrored left-right, up-down and transposed as well: the root of a set is its first pixel
in raster order and the up-right diagonal has a link of its own, so orientation matters."""
import numpy as np

SIZES = [(64, 64), (257, 131), (300, 70)]            # (W, H)
BIG = (257, 131)                                     # the size at which `dots` has far more than 512 records


def _blank(W, H):
    return np.zeros((H, W), np.uint8)


def dots(W, H):
    m = _blank(W, H)
    m[1::2, 1::2] = 255
    return m


def ring_offsets(W, H, pitch):
    """Distances from the frame of the concentric one-pixel rectangles (the outermost at 1, so that it survives
    zero_border); the innermost may be a single row, column or pixel."""
    return list(range(1, (min(W, H) + 1) // 2, pitch))


def rings(W, H, pitch, cut=None):
    """cut = None: closed rings.  cut = "second": one pixel missing from every second ring, starting with the outermost
    (only the ring behind the first cut becomes external).  cut = "outer": one pixel missing from every ring of the outer
    half (every ring down to the first closed one is external).  The missing pixels sit in the middle of a side and walk
    round the four sides from ring to ring."""
    m = _blank(W, H)
    ks = ring_offsets(W, H, pitch)
    for i, k in enumerate(ks):
        y0, y1, x0, x1 = k, H - 1 - k, k, W - 1 - k
        m[y0, x0:x1 + 1] = 255; m[y1, x0:x1 + 1] = 255
        m[y0:y1 + 1, x0] = 255; m[y0:y1 + 1, x1] = 255
        if y1 - y0 < 2 or x1 - x0 < 2:
            continue                                 # a line or a block, not a ring: a cut would split it
        if (cut == "second" and i % 2 == 0) or (cut == "outer" and i < len(ks) // 2):
            cy, cx = (y0 + y1) // 2, (x0 + x1) // 2
            y, x = [(y0, cx), (cy, x1), (y1, cx), (cy, x0)][i % 4]
            m[y, x] = 0
    return m


def _spiral_path(W, H):
    """Cells of a rectangular spiral that starts at (1, 1), runs clockwise inwards inside the frame's one-pixel margin
    and keeps one background pixel between its windings; the second list holds the path indices at which it turns."""
    on = np.zeros((H, W), bool)

    def inside(y, x):
        return 1 <= y < H - 1 and 1 <= x < W - 1

    def can_go(y, x, dy, dx):
        y1, x1, y2, x2 = y + dy, x + dx, y + 2 * dy, x + 2 * dx
        return inside(y1, x1) and not on[y1, x1] and (not inside(y2, x2) or not on[y2, x2])

    y, x, d = 1, 1, 0
    steps = [(0, 1), (1, 0), (0, -1), (-1, 0)]
    on[y, x] = True
    path, turns, straight = [(y, x)], [], 0
    while True:
        dy, dx = steps[d]
        if can_go(y, x, dy, dx):
            y, x = y + dy, x + dx
            on[y, x] = True
            path.append((y, x))
            straight += 1
            continue
        d = (d + 1) % 4
        dy, dx = steps[d]
        if straight == 0 or not can_go(y, x, dy, dx):
            break
        turns.append(len(path) - 1)
        straight = 0
    return path, turns


def spiral(W, H, diagonal=True):
    """A one-pixel-wide spiral.  diagonal: the turning cells are taken out (never two in a row), so that consecutive arms
    touch through a corner only and the whole is one 8-connected component of many 4-connected pieces."""
    path, turns = _spiral_path(W, H)
    m = _blank(W, H)
    for y, x in path:
        m[y, x] = 255
    last = -2
    for i in turns if diagonal else []:
        if i > last + 1 and 0 < i < len(path) - 1:
            m[path[i]] = 0
            last = i
    return m


def spiral_inv(W, H):
    """The complement of the 4-connected spiral: the background is a one-pixel corridor that winds to the centre and
    reaches the frame only where zero_border opens (0, 1) above its first cell."""
    return (255 - spiral(W, H, diagonal=False)).astype(np.uint8)


def comb(W, H, base_row):
    """Vertical one-pixel teeth at every second column hanging from one row.  base_row = 1: a comb inside the frame;
    base_row = 0: the joining row lies on the frame, and zero_border cuts every tooth loose.  (Mirrored up-down the teeth
    join on their last row only.)"""
    m = _blank(W, H)
    m[base_row, :] = 255
    m[base_row:H - 2, 1::2] = 255
    return m


def stairs(W, H):
    """x = 3y mod W: isolated pixels, three columns apart from row to row; x = (W-1-y) mod W: a one-pixel diagonal that
    holds together through up-right corners only."""
    m = _blank(W, H)
    y = np.arange(H)
    m[y, (3 * y) % W] = 255
    m[y, (W - 1 - y) % W] = 255
    return m


def checker(W, H):
    yy, xx = np.mgrid[0:H, 0:W]
    return (((yy + xx) % 2 == 0) * 255).astype(np.uint8)


def border(W, H, notched=True):
    """Foreground on all four frame edges and in the corners, a second ring two pixels inside with pixels of its own
    inside, and short runs that start on each edge.  notched: one-pixel background notches in every edge let the
    background in; without them the frame's ring is closed and (zero_border = False) no background touches the frame."""
    m = _blank(W, H)
    m[0, :] = m[-1, :] = 255
    m[:, 0] = m[:, -1] = 255
    if min(W, H) >= 9:
        m[2, 2:W - 2] = m[H - 3, 2:W - 2] = 255
        m[2:H - 2, 2] = m[2:H - 2, W - 3] = 255
        m[4:H - 4:2, 4:W - 4:3] = 255
        m[H // 2, 0:2] = 255                                 # joins the frame's ring and the inner ring on the left edge
    if notched:
        if min(W, H) >= 9:
            m[2, W // 2] = 0                                     # and the inner ring open as well
        for x in (1, W // 3, 2 * W // 3, W - 2):
            m[0, x] = 0
        for x in (W // 4, W // 2):
            m[-1, x] = 0
        for y in (H // 3, H - 2):
            m[y, 0] = 0
        for y in (1, H // 2, H // 2 + 1):
            m[y, -1] = 0
    return m


def noise(W, H, density, seed):
    rng = np.random.default_rng(seed)
    return ((rng.random((H, W)) < density) * 255).astype(np.uint8)


QUILT_SIDE, QUILT_PITCH, QUILT_SEEDED = 384, 8, 96


def quilt(density, seed):
    """7x7 random tiles at pitch 8 (a one-pixel background grid between them); QUILT_SEEDED of the 48 x 48 tiles hold a
    5x5 ring with a centre pixel instead, so that enclosed components certainly exist."""
    rng = np.random.default_rng(seed)
    n = QUILT_SIDE // QUILT_PITCH
    m = _blank(QUILT_SIDE, QUILT_SIDE)
    ring = np.zeros((7, 7), np.uint8)
    ring[1:6, 1:6] = 255; ring[2:5, 2:5] = 0; ring[3, 3] = 255
    seeded = set(rng.choice(n * n, QUILT_SEEDED, replace=False).tolist())
    for ty in range(n):
        for tx in range(n):
            tile = ring if ty * n + tx in seeded else ((rng.random((7, 7)) < density) * 255).astype(np.uint8)
            m[ty * 8 + 1:ty * 8 + 8, tx * 8 + 1:tx * 8 + 8] = tile
    return m


def runs(W, H, seed, longest):
    """Rows of alternating background / foreground runs with lengths in [1, longest]."""
    rng = np.random.default_rng(seed)
    m = _blank(W, H)
    for y in range(H):
        x, v = 0, int(rng.integers(0, 2))
        while x < W:
            n = int(rng.integers(1, longest + 1)) if rng.random() < 0.2 else int(rng.integers(1, 6))
            m[y, x:x + n] = 255 * v
            x += n; v ^= 1
    return m


def orientations(name, m):
    """The mask, mirrored left-right, mirrored up-down and transposed; copies that repeat an earlier one are dropped."""
    out = []
    for tag, a in (("", m), ("/lr", m[:, ::-1]), ("/ud", m[::-1, :]), ("/t", m.T)):
        a = np.ascontiguousarray(a)
        if not any(a.shape == b.shape and np.array_equal(a, b) for _, b in out):
            out.append((name + tag, a))
    return out


def _build():
    cases = []
    for W, H in SIZES:
        sz = "%dx%d" % (W, H)
        base = [("dots", dots(W, H)),
                ("rings2", rings(W, H, 2)), ("rings3", rings(W, H, 3)),
                ("rings_cut2", rings(W, H, 2, "second")), ("rings_cut3", rings(W, H, 3, "second")),
                ("rings_cut_outer2", rings(W, H, 2, "outer")),
                ("spiral", spiral(W, H)), ("spiral_inv", spiral_inv(W, H)),
                ("comb", comb(W, H, 1)), ("comb_edge", comb(W, H, 0)),
                ("stairs", stairs(W, H)), ("checker", checker(W, H)),
                ("border", border(W, H)), ("border_closed", border(W, H, notched=False)),
                ("noise45", noise(W, H, 0.45, 7 * W + H)), ("noise60", noise(W, H, 0.6, 11 * W + H))]
        for name, m in base:
            cases += orientations("%s-%s" % (name, sz), m)
    for i, density in enumerate((0.3, 0.5, 0.7)):
        cases += orientations("quilt%d-384x384" % round(density * 10), quilt(density, 300 + i))
    for W, H, longest in [(8192, 4, 700), (8191, 3, 700), (255, 5, 90), (256, 5, 90), (257, 5, 90), (511, 5, 300), (513, 5, 300),
                          (1025, 5, 600), (1, 40, 4), (40, 1, 4)]:
        cases += orientations("wide-%dx%d" % (W, H), runs(W, H, 1000 + W + H, longest))
    names = [n for n, _ in cases]
    assert len(set(names)) == len(names)
    return cases


CASES = _build()
NAMES = [n for n, _ in CASES]
BY_NAME = dict(CASES)


def family(name):
    return name.split("-")[0]


def paint(mask):
    """RGB frame whose red filter response (HSV_LOW / HSV_HIGH) is exactly `mask`: one in-range red, one gray."""
    rgb = np.empty(mask.shape + (3,), np.uint8)
    rgb[...] = (128, 128, 128)                       # s = 0
    rgb[mask != 0] = (200, 20, 20)                   # h = 0, s = 229, v = 200
    return rgb


# ---- HSV frames ------------------------------------------------------------------------------------------------------
def _rotate(vmax, a, b, sector):
    """(max, next, next-but-one channel) -> RGB columns with the maximum in channel `sector`."""
    cols = [vmax, a, b]
    return np.stack(cols[3 - sector:] + cols[:3 - sector], -1)


def hue_block():
    """For each sector (maximum in r, g, b), each diff in 0..255 and each signed offset in -diff..diff (the difference of
    the other two channels, in the order the hue formula takes it): the pixel with vmin = 0 and the one with vmin =
    255 - diff.  Offsets of +-diff make two channels tie for the maximum; the ties stay as they fall."""
    diff = np.repeat(np.arange(256), 2 * np.arange(256) + 1)
    off = np.concatenate([np.arange(-d, d + 1) for d in range(256)])
    out = []
    for sector in range(3):
        for vmin in (np.zeros_like(diff), 255 - diff):
            a = vmin + np.maximum(off, 0)            # offset = a - b, min(a, b) = vmin
            b = vmin + np.maximum(-off, 0)
            out.append(_rotate(vmin + diff, a, b, sector))
    return np.concatenate(out).astype(np.uint8)


SAT_W, SAT_H = 257, 384


def sat_block():
    """Every (v, vmin) with vmin <= v, the third channel half way between them, the maximum in r, then g, then b."""
    v, vmin = np.nonzero(np.tri(256, dtype=bool))
    return np.concatenate([_rotate(v, (v + vmin) // 2, vmin, s) for s in range(3)]).astype(np.uint8)


def sat_frame():
    """The saturation block as a frame of its own (3 x 32896 = 257 x 384 pixels)."""
    return np.ascontiguousarray(sat_block().reshape(SAT_H, SAT_W, 3))


HSV_W = 1024


def hsv_frame():
    """Hue block, saturation block, gray padding up to full rows of HSV_W pixels."""
    px = np.concatenate([hue_block(), sat_block()])
    H = -(-len(px) // HSV_W)
    pad = np.full((H * HSV_W - len(px), 3), 128, np.uint8)
    return np.ascontiguousarray(np.concatenate([px, pad]).reshape(H, HSV_W, 3))


def random_ranges(n=32, seed=77):
    """n (low, high) triples: the default red filter, one with low > high in a channel, the rest seeded random (wide and
    narrow bands, values above 180 in h)."""
    rng = np.random.default_rng(seed)
    out = [((0, 150, 0), (9, 255, 255)), ((20, 40, 200), (90, 255, 100))]
    while len(out) < n:
        lo = rng.integers(0, (190, 200, 200)) // rng.choice([1, 2, 8], 3)
        hi = lo + rng.integers(0, 256, 3) // rng.choice([1, 1, 4], 3)
        out.append((tuple(int(v) for v in lo), tuple(int(min(v, 255)) for v in hi)))
    return out
