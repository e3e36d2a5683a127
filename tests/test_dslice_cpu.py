"""The disparity-sliced search (k_search_dslice in k_search_generic.hip) on the CPU side.

1. The oracle against the brute-force model at numDisparities > 256 (the ground the sliced kernel opens), negative minD,
   thresholds on: the yardstick the GPU tests compare against is itself pinned there.
2. A NumPy model of the kernel's per-pixel fold over slices of DT reversed disparity indices against direct selection
   over the whole range, on random and adversarial cost vectors.
"""
import numpy as np
import pytest

import bruteforce as bf

BIG = 0x7FFFFFFF


@pytest.mark.parametrize("D,minD,W,H", [(272, -9, 300, 22), (512, -40, 540, 20)])
def test_oracle_matches_bruteforce_beyond_256(oracle, synth, D, minD, W, H):
    L, R = synth.make_pair(synth.STREAM_SEED + D, W, H, D)
    kw = dict(numDisparities=D, blockSize=7, minDisparity=minD, textureThreshold=10, uniquenessRatio=10,
              speckleWindowSize=20, speckleRange=32, disp12MaxDiff=1)
    a = oracle.bm_compute(L, R, **kw)
    assert np.array_equal(a, bf.stereo_bm(L, R, **kw))
    assert (a != (minD - 1) * 16).any()


def fold(S, DT):
    """The kernel's fold, slice by slice in index order -> (m, i, U, S[i-1], S[i+1]) with the end substitutions left to
    the caller (S[i+1] is BIG when i is the last index)."""
    D = len(S)
    m = i = U = Sm = Sp = P = last = None
    for E in range(0, D, DT):
        s = [int(v) for v in S[E:E + DT]]
        DL = len(s)
        sm = min(s)
        si = s.index(sm)                         # first minimum of the slice
        nw = E == 0 or sm < m
        win = E + si if nw else i
        ured = min([v for e, v in enumerate(s) if abs(E + e - win) > 1], default=BIG)
        pred = min(s[:DL - 1], default=BIG)
        Pp, lastp = (P, last) if E > 0 else (BIG, BIG)
        if nw:
            m, i = sm, win
            U = min(ured, Pp if i == E else min(Pp, lastp))
            Sm = lastp if i == E else s[i - E - 1]
            Sp = s[i - E + 1] if i - E + 1 < DL else BIG
        else:
            U = min(U, ured)
            if i == E - 1:
                Sp = s[0]
        P, last = min(Pp, lastp, pred), s[DL - 1]
    return m, i, U, Sm, Sp


def select_direct(S, uniq):
    """oracle/bm_oracle.c's selection loop over the whole range (without the texture test)."""
    D = len(S)
    mind = int(np.argmin(S))
    minsad = int(S[mind])
    ok = True
    if uniq > 0:
        thresh = minsad + minsad * uniq // 100
        ok = not any(S[d] <= thresh for d in range(D) if d < mind - 1 or d > mind + 1)
    pp = int(S[mind + 1]) if mind + 1 < D else int(S[D - 2])
    nn = int(S[mind - 1]) if mind > 0 else int(S[1])
    return mind, minsad, ok, pp, nn


def select_folded(S, DT, uniq):
    D = len(S)
    m, i, U, Sm, Sp = fold(S, DT)
    ok = uniq <= 0 or U > m + m * uniq // 100
    pp = Sp if i + 1 < D else Sm
    nn = Sm if i > 0 else Sp
    return i, m, ok, pp, nn


def _vectors(rng, D):
    yield rng.integers(0, 5000, D)
    yield rng.integers(0, 4, D)                              # many ties
    yield np.full(D, 7)                                      # all equal: index 0 wins
    for DT in (16, 32, 48):
        for pos in sorted({min(D - 1, q) for q in (0, D - 1, DT - 1, DT, DT + 1, 2 * DT - 1, 2 * DT)}):
            v = rng.integers(100, 200, D)
            v[pos] = 10                                      # a single winner on or next to a slice edge
            yield v
            v = v.copy()
            v[(pos + 2) % D] = 11                            # a near-equal rival just outside the neighbourhood
            yield v
            v = v.copy()
            v[(pos + 1) % D] = 10                            # a tie right after the winner
            yield v
    per = np.tile(np.array([5] + [50] * 15), D // 16)        # equal minima at every 16th index
    yield per


@pytest.mark.parametrize("D", [16, 32, 48, 272, 512, 4080])
@pytest.mark.parametrize("DT", [16, 32, 48, 64, 400])
def test_fold_equals_direct_selection(D, DT):
    rng = np.random.default_rng(D * 7 + DT)
    n = 0
    for S in _vectors(rng, D):
        S = np.asarray(S, np.int64)
        for uniq in (0, 10, 50):
            assert select_folded(S, DT, uniq) == select_direct(S, uniq), (D, DT, uniq, S.tolist())
            n += 1
    assert n > 30
