"""The families of tests/hostile_pairs.py do what they claim -- checked against the oracle alone (its prefilter, its whole
pipeline) and plain numpy SADs, at the route shapes that tests/test_gpu_search_hostile.py runs on the device.  Every threshold
below is a condition a family has to meet to be worth running, not a measurement."""
import functools

import numpy as np
import pytest

import hostile_cases as hc
import hostile_pairs as hp
from test_gpu_search_routes import ROWS
from test_ring_pair_cpu import LWD, RWD, prefix_ring_window_sums

ROWS7 = [r[:7] for r in ROWS]
IDS = ["%dx%d-D%d-w%d-minD%d-cap%d-legacy%d" % r for r in ROWS7]
OFF = dict(uniquenessRatio=0, textureThreshold=0, speckleWindowSize=0, disp12MaxDiff=-1)


def okw(row, cap=None):
    W, H, D, w, minD, c = row[:6]
    return dict(numDisparities=D, blockSize=w, minDisparity=minD, preFilterCap=cap or c)


def compute(oracle, row, L, R, cap=None, **kw):
    oracle.set_legacy_right_clamp(bool(row[6]))
    try:
        return oracle.bm_compute(L, R, **okw(row, cap), **kw)
    finally:
        oracle.set_legacy_right_clamp(False)


def inner_rect(W, H, D, w, minD):
    """The pixels whose left window and every right window of the range lie inside the frame: (x0, x1, y0, y1).  (The
    oracle's valid rectangle is this one where minDisparity >= 0; below 0 its last -minD columns clamp at the right edge.)"""
    r = w // 2
    return max(0, minD + D - 1) + r, min(W, W + minD) - r, r, H - r


def sad_volume(Lp, Rp, D, w, minD):
    """S[i, y - y0, x - x0]: the w x w SAD of reversed index i (disparity minD + D - 1 - i) at every pixel of inner_rect."""
    H, W = Lp.shape
    x0, x1, y0, y1 = inner_rect(W, H, D, w, minD)
    r = w // 2
    S = np.empty((D, y1 - y0, x1 - x0), np.int32)
    a = Lp[:, x0 - r:x1 + r].astype(np.int32)
    for i in range(D):
        d = minD + D - 1 - i
        c = np.abs(a - Rp[:, x0 - r - d:x1 + r - d].astype(np.int32))
        c = np.pad(c, ((1, 0), (1, 0))).cumsum(0).cumsum(1)
        S[i] = c[w:, w:] - c[:-w, w:] - c[w:, :-w] + c[:-w, :-w]
    return S


def prefiltered(oracle, L, R, cap):
    return oracle.prefilter_xsobel(L, cap), oracle.prefilter_xsobel(R, cap)


# ---- worst ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", ROWS7, ids=IDS)
def test_worst_holds_the_largest_sad_a_window_can_hold(oracle, row):
    W, H, D, w, minD, cap = row[:6]
    residues = set()
    for cap_ in sorted({cap, hc.MAXCAP[row]}):
        for seed in range(8):
            L, R = hp.make("worst", seed, W, H, D, minD, w)
            Lp, Rp = prefiltered(oracle, L, R, cap_)
            # (the prefilter writes cap into the first and last column, and into the last row of a frame of odd height)
            He = H & ~1
            assert set(np.unique(Lp[:He, 1:W - 1])) | set(np.unique(Rp[:He, 1:W - 1])) == {0, 2 * cap_}
            if seed >= 4 and cap_ != cap:
                continue
            S = sad_volume(Lp[:He], Rp[:He], D, w, minD)[:, :, 1:-1]         # windows that see neither of those columns
            d = minD + D - 1 - np.arange(D)
            top, zero = (d - hp.worst_shift(seed)) % 4 == 0, (d - hp.worst_shift(seed)) % 4 == 2
            assert top.sum() >= D // 4 and S.shape[1] > 0 and S.shape[2] > 0
            assert (S[top] == 2 * cap_ * w * w).all() and (S[zero] == 0).all()
            residues.add(int(np.flatnonzero(top)[0]) % 4)
    assert residues == {0, 1, 2, 3}                          # the saturated reversed indices fall in every residue over the seeds


# ---- worst_noise ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", ROWS7, ids=IDS)
def test_worst_noise_runs_at_the_bound_next_to_real_minima(oracle, row):
    W, H, D, w, minD, cap = row[:6]
    for seed in (0, 1):
        L, R = hp.make("worst_noise", seed, W, H, D, minD, w)
        Lp, Rp = prefiltered(oracle, L, R, cap)
        S = sad_volume(Lp[:H & ~1], Rp[:H & ~1], D, w, minD)
        rng = np.random.default_rng(77)
        ys, xs = rng.integers(0, S.shape[1], 300), rng.integers(0, S.shape[2], 300)
        share = float((S[:, ys, xs].max(0) == 2 * cap * w * w).mean())
        valid = float((compute(oracle, row, L, R) != (minD - 1) * 16).mean())
        print("worst_noise %s seed %d: %.3f of 300 windows hold the maximal SAD, %.3f of the pixels are valid" % (row, seed, share, valid))
        assert share >= 0.25
        assert valid >= 0.05


# ---- edges ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", ROWS7, ids=IDS)
def test_edges_puts_the_winners_on_both_ends_of_the_range(oracle, row):
    W, H, D, w, minD, cap = row[:6]
    fil = (minD - 1) * 16
    x0, x1, y0, y1 = inner_rect(W, H, D, w, minD)
    He = H & ~1
    for seed in (0, 1):
        L, R = hp.make("edges", seed, W, H, D, minD, w)
        first = sad_volume(*(p[:He] for p in prefiltered(oracle, L, R, cap)), D, w, minD).argmin(0)    # the winning reversed index
        for name, kw in (("off", OFF), ("default", {})):
            m = compute(oracle, row, L, R, **kw)
            v = m[m != fil].astype(np.int64)
            share = {e: float((v == dd * 16).mean()) for e, dd in (("minD", minD), ("maxD", minD + D - 1))}
            print("edges %s seed %d %s: %.3f valid, %.3f at minD, %.3f at maxD" % (row, seed, name, v.size / m.size, share["minD"], share["maxD"]))
            assert v.size / m.size > 0.05
            assert share["minD"] >= 0.10 and share["maxD"] >= 0.10, name
            # wherever an end of the range wins, the sub-pixel step reads the same neighbour twice (S[D - 2] / S[1]): p == n,
            # and the pixel is a whole one
            mi = m[y0:He - w // 2, x0:x1]
            for e, idx, dd in (("minD", D - 1, minD), ("maxD", 0, minD + D - 1)):
                at = mi[(first == idx) & (mi != fil)]
                assert at.size >= 0.10 * v.size and (at == dd * 16).all(), (e, name)


# ---- ties -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", ROWS7, ids=IDS)
def test_ties_resolve_to_the_largest_disparity_of_the_period(oracle, row):
    W, H, D, w, minD, cap = row[:6]
    r, maxD = w // 2, minD + D - 1
    x0v, x1v, y0v, y1v = inner_rect(W, H, D, w, minD)
    seen = set()
    for seed in range(6):
        L, R = hp.make("ties", seed, W, H, D, minD, w)
        assert np.array_equal(L, R)
        m = compute(oracle, row, L, R, **OFF).astype(np.int64)
        for bx0, bx1, p in hp.ties_blocks(seed, W, D, w):
            # the pixels of the block whose left window and whole search lie inside it
            xa, xb = max(x0v, bx0 + maxD + r + 1), min(x1v, bx1 - r - 1 + min(minD, 0))
            if p > D or xb <= xa:
                continue
            want = maxD - maxD % p                           # the largest d <= maxD that is congruent to 0 mod p
            assert want >= minD
            # The nearest whole disparity: the exact value want * 16 is not attainable.  The tied minimum is 0, but its two
            # neighbours are SADs of the pattern against itself shifted by +1 and by -1, which differ for a pattern that is not
            # symmetric: p != n, and the sub-pixel step moves the value by (p - n) * 128 / max(p, n) / 16, 1-2 sixteenths here.
            share = float(((m[y0v:y1v & ~1, xa:xb] + 8) >> 4 == want).mean())
            print("ties %s seed %d period %d columns [%d, %d): %.3f at disparity %d" % (row, seed, p, xa, xb, share, want))
            assert share >= 0.80
            seen.add(p)
    assert len(seen) >= (3 if D <= 64 else 2), seen           # several periods over the seeds, even where one block fits


# ---- the thresholds used on the device are live -----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _pair(family, seed, W, H, D, minD, w):
    return hp.make(family, seed, W, H, D, minD, w)


@pytest.mark.parametrize("row", sorted(hc.PINS), ids=lambda r: "%dx%d-D%d-w%d-minD%d-cap%d-legacy%d" % r)
def test_pinned_boundaries_are_live(oracle, row):
    W, H, D, w, minD, cap = row[:6]
    base = [r for r in ROWS7 if hc.with_cap(r, cap) == row and cap in (r[5], hc.MAXCAP[r])]
    assert base, "a pinned row is a row of the route table at its own or its largest cap"
    kinds = set()
    for name, family, seed, v in hc.PINS[row]:
        L, R = _pair(family, seed, W, H, D, minD, w)
        a, b = (compute(oracle, row, L, R, **hc.pin_params(name, u)) for u in (v, v + 1))
        n = int((a != b).sum())
        print("%s %s seed %d %s %d | %d: %d pixels differ" % (row, family, seed, name, v, v + 1, n))
        assert n >= 50, (name, family, seed, v)
        kinds.add((name, v) if name == hc.D12 else name)
    assert kinds == {hc.TEX, hc.UNIQ, (hc.D12, 0), (hc.D12, 1)}


def test_every_route_row_has_its_pins():
    for r in ROWS7:
        assert r in hc.PINS and hc.with_cap(r, hc.MAXCAP[r]) in hc.PINS
    assert len(hc.PINS) == len({hc.with_cap(r, c) for r in ROWS7 for c in (r[5], hc.MAXCAP[r])})


# ---- why synth.make_pair cannot stand in ----------------------------------------------------------------------------------
def _wave_copies(Lp, Rp, xb, D):
    """One wave's staged copies of every row, biased by one as the planes are: left bytes [xb, xb + 44), right bytes from
    xb - (D - 1) on (reversed index i of column x reads the right byte x - (D - 1) + i)."""
    return (Lp[:, xb:xb + 4 * LWD] + 1).astype(np.uint8), (Rp[:, xb - (D - 1):xb - (D - 1) + 4 * RWD] + 1).astype(np.uint8)


@pytest.mark.parametrize("cap", (31, 63))
def test_prefix_rings_without_rebasing_overflow_on_worst_only(oracle, synth, cap):
    """<64, 9, 4>, a strip one rebase too long: ring_rows_cap + w + 8 rows without any rebase.  On `worst` the model's own
    invariant -- the one k_search_ring.hip argues: no packed prefix sum leaves its 16-bit half -- breaks on every seed; on
    synth.make_pair at the same shape it holds, and so does everything else.  What the model shows beyond that: at this length
    the WINDOW sums still come out right on `worst`.  The shared piece joins a prefix sum with a 32-bit addition, so a low
    half that overflows there carries into its neighbour and the window's 32-bit subtraction borrows it back; only an
    overflow inside the one-byte masked piece (v_mqsad, 16-bit lanes) is lost, and at 2 cap per row that first happens
    on row 104 at cap 63 (the test below).  The bound the host keeps is therefore the safe side of the packed arithmetic, not its edge."""
    D, w = 64, 9
    W, H = 300, hc.ring_rows_cap(w, cap) + w + 8
    H += H & 1                                               # (an even height: the prefilter fills an odd last row with cap)
    xb = 120
    for seed in range(4):
        Lp, Rp = prefiltered(oracle, *hp.make("worst", seed, W, H, D, 0, w), cap)
        with pytest.raises(AssertionError, match="overflowed|65536"):
            prefix_ring_window_sums(*_wave_copies(Lp, Rp, xb, D), None)
        loose, want = prefix_ring_window_sums(*_wave_copies(Lp, Rp, xb, D), None, strict=False)
        assert np.array_equal(loose, want)                   # ... and yet the window sums are right at this length
        rebased, want2 = prefix_ring_window_sums(*_wave_copies(Lp, Rp, xb, D), hc.ring_rows_cap(w, cap) // 20)
        assert np.array_equal(rebased, want) and np.array_equal(want, want2) and want.max() == 2 * cap * w * w
    L, R = synth.make_pair(synth.STREAM_SEED + 31, W, H, D)
    got, want = prefix_ring_window_sums(*_wave_copies(*prefiltered(oracle, L, R, cap), xb, D), None)
    assert np.array_equal(got, want)
    assert want.max() < 2 * cap * w * w                      # natural texture never holds the bound


def test_prefix_rings_without_rebasing_lose_the_window_sums_later(oracle):
    # cap 63, 120 rows of `worst` without a rebase, twice the 59 rows above.  On even seeds a low half crosses 65536 inside
    # the one-byte masked piece on walked row 104, 45 rows past that length (an index five of whose nine columns differ: 630
    # a row, 104 x 630 = 65520), and from there the window sums are wrong; on odd seeds they are still right at 120 rows.
    D, w, cap, xb = 64, 9, 63, 120
    first_bad = {}
    for seed in range(4):
        Lp, Rp = prefiltered(oracle, *hp.make("worst", seed, 300, 120, D, 0, w), cap)
        got, want = prefix_ring_window_sums(*_wave_copies(Lp, Rp, xb, D), None, strict=False)
        bad = np.flatnonzero((got != want).reshape(len(got), -1).any(1))
        first_bad[seed] = int(bad[0]) + w - 1 if len(bad) else None
    assert first_bad == {0: 104, 1: None, 2: 104, 3: None}, first_bad


@pytest.mark.parametrize("row", [ROWS7[0], ROWS7[2], ROWS7[5]], ids=[IDS[0], IDS[2], IDS[5]])
def test_a_last_minimum_selection_fails_on_ties_only(oracle, synth, row):
    W, H, D, w, minD, cap = row[:6]
    x0, x1, y0, y1 = inner_rect(W, H, D, w, minD)
    He = H & ~1

    def shares(L, R):
        m = compute(oracle, row, L, R, **OFF).astype(np.int64)[y0:He - w // 2, x0:x1]
        S = sad_volume(*(p[:He] for p in prefiltered(oracle, L, R, cap)), D, w, minD)
        first = minD + D - 1 - S.argmin(0)
        last = minD + S[::-1].argmin(0)
        # the oracle's value lies within half a pixel of the integer winner
        return float((np.abs(m - 16 * first) > 8).mean()), float((np.abs(m - 16 * last) > 8).mean())

    for seed in (0, 1, 2):
        f, l = shares(*hp.make("ties", seed, W, H, D, minD, w))
        print("ties %s seed %d: first minimum differs on %.3f, last minimum on %.3f" % (row, seed, f, l))
        assert f == 0.0 and l >= 0.30
    f, l = shares(*synth.make_pair(synth.STREAM_SEED + 32, W, H, D))
    print("make_pair %s: first minimum differs on %.3f, last minimum on %.3f" % (row, f, l))
    assert f == 0.0 and l < 0.01
