"""Stereo pairs for the left-right check (K3) beside the families of tests/hostile_pairs.py.  Pure numpy, seeded, no device.
Conventions as there: disparity d means L[y, x] == R[y, x - d].

  sawtooth     L = (x % 32) * 8, R = 255 - (x % 32) * 8, row-constant, a share `noise` of the pixels of each view replaced by
               uint8 noise.  The x-Sobel response of the two views has opposite signs almost everywhere, so the best window
               still costs most of 2 cap w w: winners whose SAD has its top bits set, next to the cheap ones around the noise.
  cliffs       independent uint8 noise in both views; every block (x0, x1, d) makes L[:, x0:x1] a copy of R at disparity d.
               Blocks may claim the same right columns hundreds of disparities apart.
  nonvoter     the one column per row that holds a disparity but may not vote, set up so that its vote would be seen.
  nonvoter_ramp  a ramp of disparities whose pixels all look up the slot that holds that column's vote and no other.
  straddle     column blocks two disparities apart around a disparity d, so that the two claimants of a right column lie
               on either side of 16 d.
  range_steps  every left column is a copy of the right view: wide anchors at disparity d0 that alternate with narrow strips
               at d0 + 256 and d0 + 257 in turn (a period of 64 columns, so that no two left columns claim one right column
               but for the one column by which 257 misses a multiple of the period), and a little noise of the right view's
               own, which moves the sub-pixel parts by a few sixteenths.  Neighbours across an anchor | strip boundary differ
               by 4096 or 4112 give or take those sixteenths -- what speckleRange 4095 | 4096 | 4097 decides.
"""
import numpy as np

CLIFF_BLOCKS = ((700, 800, 60), (1212, 1312, 572), (810, 900, 50), (1330, 1400, 570))
RS_PERIOD, RS_STRIP = 64, 16


def sawtooth(seed, W, H, noise=0.01):
    rng = np.random.default_rng([int(seed), 21])
    ramp = ((np.arange(W) % 32) * 8).astype(np.uint8)
    L, R = np.tile(ramp, (H, 1)), np.tile((255 - ramp).astype(np.uint8), (H, 1))
    for img in (L, R):
        m = rng.random((H, W)) < noise
        img[m] = rng.integers(0, 256, int(m.sum()), dtype=np.uint8)
    return L, R


def cliffs(seed, W, H, blocks=CLIFF_BLOCKS):
    rng = np.random.default_rng([int(seed), 22])
    L = rng.integers(0, 256, (H, W), dtype=np.uint8)
    R = rng.integers(0, 256, (H, W), dtype=np.uint8)
    for x0, x1, d in blocks:
        assert 0 <= x0 - d and x0 < x1 <= W, (x0, x1, d)
        L[:, x0:x1] = R[:, x0 - d:x1 - d]
    return L, R


def nonvoter(seed, W, H, D, w, d_nv=5, rough=0.4):
    """minDisparity 0.  Independent noise, but for two pieces of the left view that show the same piece of the right view:
    the window around column D - 1 -- the one column per row that the search computes and that may not vote, a NON-VOTER --
    at disparity d_nv, so that its vote, if it had one, would go into slot s = D - 1 - d_nv; and a block a window wide around
    a column p inside the valid rectangle, roughened (bit 6 of a share `rough` of its pixels flipped) so that p's cost is
    above the non-voter's.  p is the only voter of slot s and finds itself there; where a non-voter's vote counts, the
    cheaper non-voter takes the slot and p finds a disparity that is not its own -- in the rows where p's disparity is at or
    a sixteenth below a whole number, so that its other look-up is slot s + 1, which the non-voter's right neighbour wins."""
    rng = np.random.default_rng([int(seed), 24])
    L = rng.integers(0, 256, (H, W), dtype=np.uint8)
    R = rng.integers(0, 256, (H, W), dtype=np.uint8)
    r, x_nv = w // 2, D - 1
    s = x_nv - d_nv
    x_p = x_nv + w + 3 + r                                  # clear of the non-voter's window, r columns inside the rectangle
    k = x_p - s
    assert s - r - 2 >= 0 and k + 1 <= D - 1 and x_p + w + 2 <= W, (s, k, D)
    # the non-voter: its window hangs over the search's left edge, where the right view's columns are clamped -- flat to its
    # left and a right column s between equal neighbours keep the cost of that small
    R[:, s + 1] = R[:, s - 1]
    L[:, :x_nv] = 128
    L[:, x_nv:x_nv + r + 2] = R[:, s:s + r + 2]
    cols = np.arange(x_p - r - 1, x_p + r + 2)
    block = R[:, cols - k]
    L[:, cols] = block ^ ((rng.random(block.shape) < rough).astype(np.uint8) * 64)
    return L, R


def nonvoter_ramp(seed, W, H, D, w):
    """minDisparity 0.  Look-ups of a slot that holds a non-voter's vote and no other.  The right view is noise but for one flat
    block that holds exactly one flat window, centred on column c, with a hard step on its left and three columns of faint
    texture on its right.  The left view is flat from its left edge on, shows those three columns r + 1 columns right of
    column D - 1 -- the NON-VOTER, whose only zero-cost match is then at slot c + 1 -- and is flat again for c more columns:
    every flat window there matches the one flat window of the right view, so the disparity rises by one per column (all of
    them vote into slot c), and the step on the left is the stronger neighbour, which puts the sub-pixel part below the whole
    number: those pixels look up slots c + 1 and c.  Nobody votes into c + 1."""
    rng = np.random.default_rng([int(seed), 26])
    L = rng.integers(0, 256, (H, W), dtype=np.uint8)
    R = rng.integers(0, 256, (H, W), dtype=np.uint8)
    r, x_nv = w // 2, D - 1
    c = min(40, D - 4)
    assert c - r - 2 >= 0 and x_nv + c + r + 2 <= W
    R[:, c - r - 1:c + r + 2] = 100
    R[:, c - r - 2] = 255
    faint = (100 + rng.integers(-2, 3, (H, 3))).astype(np.uint8)
    faint[:, 1] = np.where(np.arange(H) % 2, 97, 103)        # never flat
    R[:, c + r + 2:c + r + 5] = faint
    L[:, :x_nv + c + r + 2] = 100
    L[:, x_nv + r + 1:x_nv + r + 4] = faint
    return L, R


def straddle(seed, W, H, d=-1024, block=8, flips=0.05):
    """Column blocks of the left view at disparity d - 1 and d + 1 in turn (negative: the right view is the left one moved
    right), with a little noise of the right view's own.  Where the disparity rises by two, two left columns claim one right
    column from either side of 16 d: the loser finds a disparity two away from its own (disp12MaxDiff 2 lets it live)."""
    rng = np.random.default_rng([int(seed), 25])
    L = rng.integers(0, 256, (H, W), dtype=np.uint8)
    R = rng.integers(0, 256, (H, W), dtype=np.uint8)
    for x in range(W):
        t = x - (d + (1 if (x // block) & 1 else -1))
        if 0 <= t < W:
            R[:, t] = L[:, x]
    R ^= (rng.random((H, W)) < flips).astype(np.uint8) * 8
    return L, R


def range_steps_disparities(W, d0, period=RS_PERIOD, strip=RS_STRIP):
    """the disparity of every left column: anchors d0, strips d0 + 256 and d0 + 257 in turn (none left of column d0 + 257 + 16)"""
    d = np.full(W, d0, np.int64)
    k = 0
    for x0 in range(period - strip, W - strip, period):
        if x0 - (d0 + 257) < 16:
            continue
        d[x0:x0 + strip] = d0 + 256 + (k & 1)
        k += 1
    return d


def range_steps(seed, W, H, d0=6, flips=0.05, period=RS_PERIOD, strip=RS_STRIP):
    rng = np.random.default_rng([int(seed), 23])
    R = rng.integers(0, 256, (H, W), dtype=np.uint8)
    x = np.arange(W)
    src = x - range_steps_disparities(W, d0, period, strip)
    L = rng.integers(0, 256, (H, W), dtype=np.uint8)
    ok = src >= 0
    L[:, ok] = R[:, src[ok]]
    R = R ^ ((rng.random((H, W)) < flips).astype(np.uint8) * 8)
    return L, np.ascontiguousarray(R)
