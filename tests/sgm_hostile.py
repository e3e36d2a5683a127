"""Deterministic stereo pairs that reach the cases the StereoSGBM kernels are built around (oracle/sgm_oracle.c, rules R5 - R9),
where natural pairs stay far from them.  Pure numpy, seeded, no device.

    make(family, seed, W, H, D, minD=0) -> (L, R)     uint8 [H, W]
    make_n(family, seed, n, W, H, D, minD=0)          uint8 [n, H, W]: frame i is make(family, seed + i, ...)

Conventions as in hostile_pairs.py: disparity d means L[y, x] == R[y, x - d]; costs live on the columns [max(minD + D, 0),
W + min(minD, 0)) and the disparity INDEX is d - minD in [0, D).  Each family is meant for a parameter set (blockSize, P1, P2 per
mode: tests/sgm_hostile_cases.py); tests/test_sgm_hostile_cpu.py asserts what each one claims.

Families:
  partial_sat  noise against its copy, shifted by another in-range disparity in every band of rows, with column blocks of
               unrelated noise in the left view.  With P1 / P2 of several thousand at blockSize 9 most non-winning aggregated
               costs saturate at 32767 (R5) while the winners do not: the saturated S[d +- 1] enter the sub-pixel formula,
               min(S + L_r, 32767) is live in every pass, and in MODE_HH every cost of some pixels saturates (no winner).
  at_limit     partial_sat's content without the unrelated blocks and with a few flipped bits.  Its P2 is computed FROM THE FRAME,
               sgm_hostile_ref.limit_P2: 32767 - the largest block cost, so the frame is accepted and refused at P2 + 1 (deviation (a)), and a
               path cost reaches 32767 exactly.
  ties         hostile_pairs.worst: period 4, every aggregated cost ties with the one four disparities on.
  ties35       L == R up to a shift per band of rows, row-constant, the sum of a period-3 and a period-5 pattern: costs tie 15
               disparities apart (near-ties 3, 5, 6, 9, 10 and 12 apart), the first minimum anywhere in [0, 15) -- the tied
               minima sit in different lanes at 2, 4, 8 and 16 disparities per lane, in different 16-lane rows from D = 128 on
               and in different waves at D = 1040.
  vote_ties    two grey levels; the right view is the left one under a disparity that rises by one every two to four columns
               (flat where no left pixel lands), so the left pixels beside a step claim one right column, with EQUAL minS (few
               distinct costs at blockSize 1 and the smallest P1 / P2) and different winners: R7's "the larger x stays" decides
               the vote, R9 shows it in the map.
  ends         hostile_pairs.edges in bands of two rows: winners at index 0 and D - 1 (no interpolation, the clamped
               neighbour look-up), one inside and one outside either end.
  steps        hostile_pairs.steps: two left pixels two disparities apart claim one right pixel -- disp12MaxDiff 1 | 2.
"""
import numpy as np

import hostile_pairs as hp

FAMILIES = ("partial_sat", "at_limit", "ties", "ties35", "vote_ties", "ends", "steps")
SAT = 32767


def _banded_copy(rng, L, D, minD, band, lo=2, hi=3):
    """R[y, x - d] = L[y, x] with one disparity d in [minD + lo, minD + D - hi] per band of rows; the rest of R is noise of
    its own.  -> (R, [d per band])"""
    H, W = L.shape
    R = rng.integers(0, 256, (H, W), dtype=np.uint8)
    ds = []
    for y0 in range(0, H, band):
        d = int(rng.integers(minD + lo, minD + D - hi + 1))
        ds.append(d)
        x = np.arange(W)
        ok = (x - d >= 0) & (x - d < W)
        R[y0:y0 + band, x[ok] - d] = L[y0:y0 + band, x[ok]]
    return R, ds


def partial_sat(seed, W, H, D, minD=0):
    rng = np.random.default_rng([int(seed), 21])
    L = rng.integers(0, 256, (H, W), dtype=np.uint8)
    R, _ = _banded_copy(rng, L, D, minD, band=6 + int(seed) % 3)
    # unrelated blocks: in the LEFT view, over the cost domain (what they cover has no match at any disparity)
    x0, x1 = max(minD + D, 0), W + min(minD, 0)
    x = x0 + int(rng.integers(2, 8))
    while x < x1:
        bw = int(rng.integers(3, 7))
        L[:, x:min(x + bw, x1)] = rng.integers(0, 256, (H, min(x + bw, x1) - x), dtype=np.uint8)
        x += bw + int(rng.integers(9, 17))
    return L, R


def at_limit(seed, W, H, D, minD=0):
    rng = np.random.default_rng([int(seed), 22])
    L = rng.integers(0, 256, (H, W), dtype=np.uint8)
    R, _ = _banded_copy(rng, L, D, minD, band=7 + int(seed) % 3)
    R ^= ((rng.random((H, W)) < 0.04) * 16).astype(np.uint8)
    return L, R


def ties(seed, W, H, D, minD=0):
    return hp.worst(seed, W, H, D, minD)


def ties35(seed, W, H, D, minD=0):
    rng = np.random.default_rng([int(seed), 23])
    x = np.arange(W + 15)
    L = np.empty((H, W), np.uint8)
    R = np.empty((H, W), np.uint8)
    band = 8 + int(seed) % 3
    for y0 in range(0, H, band):
        while True:
            a, b = rng.integers(0, 8, 3) * 16, rng.integers(0, 8, 5) * 16
            row = a[x % 3] + b[x % 5]                              # <= 224
            # no shorter period than 15: every shift by 3, 5, 6, 9, 10 or 12 must change the row
            if all((row != np.roll(row[:15], s)[x % 15]).any() for s in (3, 5, 6, 9, 10, 12)):
                break
        s = int(rng.integers(0, 15))                               # R[x] = L[x + s]: costs vanish at d = s mod 15
        L[y0:y0 + band] = row[:W]
        R[y0:y0 + band] = row[(np.arange(W) + s) % 15]
    if D >= 128:
        # the right view is noise from column X0 on: the last domain column sees the periodic rows only at the indices above
        # B - 8 (the columns before it from lower indices on, but the horizontal paths carry the last one's costs to them), B the
        # largest power of two <= D / 2, so the first minimum lies within 8 of B -- the boundary between the 16-lane rows of a
        # half-wave (D = 128: 64, D = 256: 128), of a wave (D = 272: 128) and between two waves (D = 1040: 512) -- and the tied
        # one 15 further
        B = 1 << ((D // 2).bit_length() - 1)
        X0 = (W + min(minD, 0) - 1) - minD - (B - 8)
        R[:, X0:] = rng.integers(0, 256, (H, W - X0), dtype=np.uint8)
    return L, R


def vote_ties(seed, W, H, D, minD=0):
    rng = np.random.default_rng([int(seed), 24])
    lv = np.array([64, 192], np.uint8)
    L = lv[rng.integers(0, 2, (H, W))]
    R = np.full((H, W), 64, np.uint8)                              # flat where no left pixel lands
    lo, hi = minD + 1, minD + D - 2
    for y0 in range(0, H, 4):                                      # bands of four rows, each with its own staircase
        d = lo + int(rng.integers(0, max(1, hi - lo)))
        nxt = int(rng.integers(2, 5))
        for xx in range(W):                                        # left to right: the nearer surface overwrites the farther
            if xx == nxt:
                d = d + 1 if d + 1 <= hi else lo
                nxt += int(rng.integers(2, 5))
            if 0 <= xx - d < W:
                R[y0:y0 + 4, xx - d] = L[y0:y0 + 4, xx]
    return L, R


def ends(seed, W, H, D, minD=0):
    return hp.edges(seed, W, H, D, minD, 1)                        # w = 1: bands of two rows, all six steps from H = 12 on


def steps(seed, W, H, D, minD=0):
    return hp.steps(seed, W, H, D, minD, 5)


_MAKERS = dict(partial_sat=partial_sat, at_limit=at_limit, ties=ties, ties35=ties35, vote_ties=vote_ties, ends=ends, steps=steps)


def make(family, seed, W, H, D, minD=0):
    L, R = _MAKERS[family](int(seed), int(W), int(H), int(D), int(minD))
    L, R = np.ascontiguousarray(L, np.uint8), np.ascontiguousarray(R, np.uint8)
    assert L.shape == R.shape == (H, W)
    return L, R


def make_n(family, seed, n, W, H, D, minD=0):
    pairs = [make(family, int(seed) + i, W, H, D, minD) for i in range(n)]
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


def colour(L, R, seed):
    """An interleaved colour pair [H, W, 3] from a gray one: the gray plane and two planes derived from it (the same
    correspondence in all three)."""
    rng = np.random.default_rng([int(seed), 25])
    lut = rng.integers(0, 256, (2, 256), dtype=np.uint8)
    return np.stack([L, lut[0][L], lut[1][L]], -1), np.stack([R, lut[0][R], lut[1][R]], -1)
