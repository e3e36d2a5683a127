"""The inputs of test_gpu_sgm_3way.py, shared with test_sgm_3way_cpu.py, which asserts without a GPU what the GPU cases rest on
(the reference finds disparities, four stripes differ from one, T3's floor shows), so that no GPU case can pass vacuously."""
import numpy as np

import sgm_3way_ref as ref

NOISE = 40


def pair(seed, W, H, shift, cn=1, noise=NOISE):
    """A textured pair whose right view is the left one moved by `shift` columns, gray (H x W) or colour (H x W x 3), each view
    with noise of its own (+-noise, uniform): enough ambiguity that the path costs, not the block costs alone, pick the winners --
    so a change in the vertical paths (stripes, T3's floor) shows in the map."""
    rng = np.random.default_rng(seed)
    T = rng.integers(0, 256, (H, W + abs(shift), cn)).astype(np.float64)
    T = (T + np.roll(T, 1, 1) + np.roll(T, -1, 1) + np.roll(T, 1, 0) + np.roll(T, -1, 0)) / 5
    T = np.stack([np.clip(T + rng.integers(-noise, noise + 1, T.shape), 0, 255) for _ in range(2)]).astype(np.uint8)
    TL, T = T[0], T[1]
    if shift >= 0:
        L, R = TL[:, :W], T[:, shift:shift + W]
    else:
        L, R = TL[:, -shift:-shift + W], T[:, :W]
    L, R = L.copy(), R.copy()
    return (L[:, :, 0].copy(), R[:, :, 0].copy()) if cn == 1 else (L, R)


def three_plane_pair(seed, W, H, xb, yb, bw, da, db, dc, scale):
    """Random texture (contrast x scale) at disparity da left of column xb and db right of it, and at dc in a band of 2 bw - 1
    columns around xb above row yb.  Under a P2 far above the block costs a path keeps the disparity it has walked in with for
    many steps, so below the band's end -> arrives with da, <- with db and the downward path with dc: whichever disparity a
    pixel there takes, two of the three directions charge it most of a P2 each."""
    rng = np.random.default_rng(seed)
    R = (rng.integers(0, 256, (H, W + 16)) * scale).astype(np.uint8)
    y, x = np.mgrid[0:H, 0:W]
    d = np.where(x < xb, da, db)
    d = np.where((y < yb) & (np.abs(x - xb) < bw), dc, d)
    return R[y, x - d + 16].astype(np.uint8), R[:, 16:16 + W].copy()


def noise_pair(seed, W, H):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (H, W)).astype(np.uint8), rng.integers(0, 256, (H, W)).astype(np.uint8)


class Case:
    """One textured GPU case: a frame W x H (W1 = W - D columns of cost domain at minD = 0) and the matcher's knobs."""
    def __init__(self, name, W, H, D, bs, minD=0, cn=1, cap=0, census=None, uniq=10, spk=0, P2=2400, shift=5, noise=NOISE):
        self.name, self.W, self.H, self.D, self.bs, self.minD, self.cn, self.cap = name, W, H, D, bs, minD, cn, cap
        self.census, self.uniq, self.spk, self.P2, self.shift, self.noise = census, uniq, spk, P2, shift, noise

    def frames(self, seed=0):
        return pair(9000 + sum(map(ord, self.name)) + seed, self.W, self.H, self.minD + self.shift + 2 * seed, self.cn, self.noise)

    def warms_up(self):
        """a stripe with output rows starts below row 0: its chain warms up, on C' for blockSize > 1"""
        return any(a > 0 and o < e for a, o, e in ref.stripes(self.H, self.bs))

    def params(self):
        """keywords of the reference (and, numDisparities renamed, of the matcher)"""
        return dict(numDisparities=self.D, blockSize=self.bs, minDisparity=self.minD, uniquenessRatio=self.uniq,
                    speckleWindowSize=self.spk, P2=self.P2)

    def want(self, L, R, **kw):
        return ref.sgm_compute(L, R, preFilterCap=self.cap, census=self.census, **dict(self.params(), **kw))


# W ~ D + 40; H: 65 -> stripes of 17 rows with 5 .. 12 rows of overlap, 9 and 5 -> an overlap longer than a stripe and a = 0 for
# several stripes, 3 -> an empty fourth stripe
CASES = [
    Case("d16_odd_w1", 57, 65, 16, 5),                           # W1 = 41: the last wave's repeated half
    Case("d48_dead_lanes", 88, 20, 48, 5),
    Case("d64", 104, 33, 64, 3, spk=100),                        # the speckle filter on
    Case("d128", 168, 24, 128, 5),
    Case("d256", 296, 16, 256, 5),
    Case("h9", 56, 9, 16, 5),
    Case("h5", 56, 5, 16, 5),
    Case("h3_empty_stripe", 56, 3, 16, 5),
    Case("bs1_no_warm", 72, 33, 32, 1),
    Case("bs9_unfused", 72, 40, 32, 9),
    Case("bs19_checked", 57, 65, 16, 19, noise=70),                      # k_sgm_box_any, T8 live: 93 * 361 + 2400 > 32767
    Case("minD_m8", 80, 21, 32, 5, minD=-8),
    Case("minD_p4", 76, 21, 32, 5, minD=4),
    Case("colour", 72, 21, 32, 5, cn=3, noise=70),
    Case("cap63", 72, 21, 32, 5, cap=63),
    Case("census97", 72, 21, 32, 5, census=(9, 7), noise=70),        # (the Hamming cost shrugs off +-40; +-70 leaves the paths a say)
    Case("uniq0", 72, 21, 32, 5, uniq=0),
]
BY_NAME = {c.name: c for c in CASES}
# four stripes are asserted to give another map than one on every case with a stripe that warms up (all but h5 and h3), and
# T3's floor is asserted to show in the map on every such case that has a C' (all of those but blockSize 1)
STRIPE_CASES = tuple(c.name for c in CASES if c.warms_up())
FLOOR_CASES = tuple(c.name for c in CASES if c.warms_up() and c.bs > 1)

# every aggregated cost of some pixels saturated (R5): no winner
# (runs of 110 columns and 74 rows at ~260 a step: about 28000 and 17000 of accumulated cost -- any two pass 32767; the junction
# lies at the end of stripe 0, whose downward chain starts at row 0; block costs stay below 32767 - 32000)
SATURATED = dict(W=236, H=320, D=16, bs=5, P1=31999, P2=32000, uniq=0)


def saturated_pair():
    s = SATURATED
    return three_plane_pair(7, s["W"], s["H"], 16 + (s["W"] - 16) // 2, 74, 4, 2, 7, 12, 0.5)


def saturated_params():
    s = SATURATED
    return dict(numDisparities=s["D"], blockSize=s["bs"], P1=s["P1"], P2=s["P2"], uniquenessRatio=s["uniq"], speckleWindowSize=0)


# a pair T8 refuses: noise under blockSize 19 at P2 = 32000 (block costs of ~11000 against a limit of 767)
REFUSED = dict(W=57, H=33, D=16, bs=19, P2=32000)

# a pair T8 refuses through a C' ALONE.  blockSize 19 (R = 9), H = 65: stripe 2 starts at a = 22.  Rows [22, 31) are 255 in the
# left view and 0 in the right one, every other row 128 in both: no x-gradient anywhere, so a pixel cost is (255 - 0) >> 2 = 63
# in the band and 0 outside it (a little else where R1's overwritten border columns come in).  A frame-relative window holds at
# most the band's 9 rows: C <= 9 * 19 * 63 = 10773.  C'(22) counts row 22 ten times and rows 23 .. 30 once: 18 * 19 * 63 = 21546.
# The limit at P2 = 20000 is 12767, between the two.
WARM_REFUSED = dict(W=57, H=65, D=16, bs=19, P2=20000, band=(22, 31))


def warm_refused_pair():
    r = WARM_REFUSED
    L = np.full((r["H"], r["W"]), 128, np.uint8); R = L.copy()
    L[r["band"][0]:r["band"][1]] = 255
    R[r["band"][0]:r["band"][1]] = 0
    return L, R


def warm_refused_params():
    r = WARM_REFUSED
    return dict(numDisparities=r["D"], blockSize=r["bs"], P2=r["P2"], speckleWindowSize=0)
