"""The wide-line StereoSGBM path pass (k_sgm_wide.hip) on the CPU side.

1. The oracle against the brute-force model at numDisparities > 256 (the ground the wide pass opens), both modes: the
   yardstick the GPU tests compare against is itself pinned there.
2. A NumPy model of the wide pass's winner rule -- 12-bit key (S << 12) | d, per-lane then per-wave then cross-wave minimum,
   uniqueness votes per wave, S[d* -+ 1] read from whichever lane / wave holds them, sub-pixel -- against direct selection
   (oracle/sgm_oracle.c R6, R8), with ties on lane and wave boundaries.
"""
import numpy as np
import pytest

import bruteforce as bf


@pytest.mark.parametrize("D,paths", [(272, 8), (272, 5), (320, 8), (320, 5)])
def test_oracle_matches_bruteforce_beyond_256(oracle, synth, D, paths):
    W, H = D + 14, 6
    L, R = synth.make_pair(synth.STREAM_SEED + 60 + D + paths, W, H, 64)
    kw = dict(numDisparities=D, blockSize=3, minDisparity=-4, uniquenessRatio=5, speckleWindowSize=0, disp12MaxDiff=2,
              paths=paths)
    a = oracle.sgm_compute(L, R, **kw)
    assert np.array_equal(a, bf.sgm(L, R, **kw))
    assert (a != (-4 - 1) * 16).any()


def select_direct(S, uniq, minD=0):
    """R6 + R8 over the whole range: (d16 + minD * 16, bd + minD, mins) or None (no winner / rejected)."""
    D = len(S)
    bd = int(np.argmin(S))
    mins = int(S[bd])
    if mins >= 32767:
        return None
    far = np.abs(np.arange(D) - bd) > 1
    if np.any(far & (S.astype(np.int64) * (100 - uniq) < mins * 100)):
        return None
    d16 = bd * 16
    if 0 < bd < D - 1:
        sn, sp = int(S[bd - 1]), int(S[bd + 1])
        den = max(sn + sp - 2 * mins, 1)
        num = (sn - sp) * 16 + den
        d16 += abs(num) // (den * 2) * (1 if num >= 0 else -1)
    return d16 + minD * 16, bd + minD, mins


def select_wide(S, uniq, np2, nw, minD=0):
    """The kernel's steps: lanes of 2 * np2 disparities, 64 lanes per wave, nw waves per line; dead (padded) lanes hold
    0xffff and take no part in the key, the votes or the neighbours."""
    D = len(S)
    lpd = 2 * np2
    cap = nw * 64 * lpd
    assert cap >= D and D % 16 == 0
    Sp = np.full(cap, 0xFFFF, np.int64)
    Sp[:D] = S
    lanes = Sp.reshape(nw, 64, lpd)
    live = (np.arange(nw * 64) * lpd < D).reshape(nw, 64)
    d = np.arange(cap).reshape(nw, 64, lpd)
    keys = np.where(live[:, :, None], (lanes << 12) | d, 0x7FFFFFFF)
    assert keys.max() < 2 ** 31 and (keys[live] < 2 ** 27).all()
    lane_key = keys.min(axis=2)                      # the lane's own elements
    wave_key = lane_key.min(axis=1)                  # DPP rows + permlane16 / permlane32 swaps
    key = int(wave_key.min())                        # across waves: LDS
    mins, bd = key >> 12, key & 0xFFF
    hits = live[:, :, None] & (np.abs(d - bd) > 1) & (lanes * (100 - uniq) < mins * 100)
    rejected = bool(hits.any(axis=(1, 2)).any()) or mins >= 32767    # per-wave __any, then the waves' votes
    if rejected:
        return None
    ip, in_ = min(bd + 1, D - 1), max(bd - 1, 0)

    def fetch(i):                                    # the wave that holds i, its lane (ds_bpermute), the pair, the half
        lane = i // lpd
        w, l = lane >> 6, lane & 63
        pair = (lanes[w, l, (i % lpd) // 2 * 2] | (lanes[w, l, (i % lpd) // 2 * 2 + 1] << 16))
        return int((pair >> ((i & 1) * 16)) & 0xFFFF)
    s_p, s_n = fetch(ip), fetch(in_)
    d16 = bd * 16
    if 0 < bd < D - 1:
        den = max(s_n + s_p - 2 * mins, 1)
        num = (s_n - s_p) * 16 + den
        d16 += abs(num) // (den * 2) * (1 if num >= 0 else -1)
    return d16 + minD * 16, bd + minD, mins


def forms(D):
    out = []
    for nw in (1, 4):
        np2 = 1
        while nw * 128 * np2 < D:
            np2 *= 2
        if np2 <= 8:
            out.append((np2, nw))
    return out


@pytest.mark.parametrize("D", [16, 48, 256, 272, 336, 512, 1024, 1040, 2048, 4080])
def test_wide_winner_rule_equals_direct_selection(D):
    rng = np.random.default_rng(D)
    for trial in range(60):
        kind = trial % 4
        if kind == 0:
            S = rng.integers(0, 32768, D)
        elif kind == 1:
            S = rng.integers(2000, 2600, D)                       # near ties everywhere
        elif kind == 2:
            S = np.full(D, 32767)                                 # every cost saturated: no winner
            if trial % 8 == 6:
                S[rng.integers(0, D)] = 32766
        else:
            S = rng.integers(5000, 32768, D)
            b = int(rng.integers(0, D))
            S[b] = 100
            for n in (b - 1, b + 1):
                if 0 <= n < D:
                    S[n] = int(rng.integers(100, 400))
        uniq = int(rng.choice([0, 10, 50, 100]))
        want = select_direct(S, uniq, minD=-7)
        for np2, nw in forms(D):
            assert select_wide(S, uniq, np2, nw, minD=-7) == want, (D, trial, np2, nw)


@pytest.mark.parametrize("D", [272, 512, 1024, 2048, 4080])
def test_ties_on_lane_and_wave_boundaries(D):
    # equal minima on both sides of every lane boundary of every form and on both sides of every wave boundary: the first
    # one wins, its neighbours come from the next lane / wave
    edges = set()
    for np2, nw in forms(D):
        lpd = 2 * np2
        edges |= {e for e in range(lpd, D, lpd)}
        edges |= {e for e in range(64 * lpd, D, 64 * lpd)}
    for e in sorted(edges)[:: max(1, len(edges) // 40)]:
        for uniq in (0, 15):
            S = np.full(D, 9000)
            S[e - 1] = S[e] = 700
            if e + 1 < D:
                S[e + 1] = 900
            if e - 2 >= 0:
                S[e - 2] = 760
            want = select_direct(S, uniq)
            assert want is not None and want[1] == e - 1
            for np2, nw in forms(D):
                assert select_wide(S, uniq, np2, nw) == want, (D, e, np2, nw)
