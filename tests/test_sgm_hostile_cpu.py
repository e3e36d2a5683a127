"""The pairs of tests/sgm_hostile.py do what they claim, shown on the oracle alone (no device): saturation of some but not all
aggregated costs, the overflow rule exactly on its boundary, tied minima in different lanes / rows / waves, tied votes that the
map shows, winners on both ends of the range, the disp12MaxDiff boundary, and uniqueness pins that are live.  The seeds and
parameters recorded in tests/sgm_hostile_cases.py are re-checked here; tests/test_gpu_sgm_hostile.py runs the same frames on
every route of the device."""
import ctypes as C
import functools

import numpy as np
import pytest

import sgm_hh4_ref
import sgm_hostile as sh
import sgm_hostile_ref as hr
import sgm_hostile_cases as hc

SAT = sh.SAT
N = 3                                                   # the frames seed .. seed + 2 the device suite runs


@pytest.fixture(autouse=True)
def _oracle(oracle):
    return oracle


@functools.lru_cache(maxsize=None)
def frames(family, D, minD=0):
    W1, H = hc.shape(D)
    return sh.make_n(family, hc.seed(family, D), N, hc.width(D, minD, W1), H, D, minD)


@functools.lru_cache(maxsize=None)
def case(family, D, paths, k=0, minD=0):
    """-> (keywords, [(L, R, block costs, S)] per frame) of parameter set k"""
    Ls, Rs = frames(family, D, minD)
    kw = hr.resolve(hc.param_sets(family, paths)[k], Ls, Rs, D, minD)
    return kw, [(L, R) + tuple(hr.volumes(L, R, paths, kw)) for L, R in zip(Ls, Rs)]


def valid_share(m, D, minD=0):
    """the share of valid pixels: of the frame at D = 64, the issue's shape (0.488 of it is cost domain), of the cost domain at
    every other D (at D >= 142 the domain is less than 0.30 of the frame)"""
    W1, H = hc.shape(D)
    return float((m != (minD - 1) * 16).sum()) / (m.size if D == 64 else W1 * H)


def saturation(S):
    """-> shares: (pixels with some but not all costs at 32767, interior winners with a saturated neighbour, pixels with
    every cost saturated)"""
    D = S.shape[2]
    sat = S >= SAT
    allsat = sat.all(2)
    bd = S.argmin(2)
    yy, xx = np.nonzero((bd > 0) & (bd < D - 1) & ~allsat)
    nb = (S[yy, xx, bd[yy, xx] - 1] >= SAT) | (S[yy, xx, bd[yy, xx] + 1] >= SAT)
    return float((sat.any(2) & ~allsat).mean()), float(nb.mean()), float(allsat.mean())


def two_minima(S):
    """-> (pixels with more than one minimum [H, W1] bool, index of the first minimum, of the second)"""
    ism = S == S.min(2, keepdims=True)
    multi = ism.sum(2) > 1
    first = ism.argmax(2)
    rest = ism.copy()
    np.put_along_axis(rest, first[:, :, None], False, 2)
    return multi, first, np.where(multi, rest.argmax(2), first)


def apart(S, group):
    """pixels whose first and second minimum lie in different groups of `group` consecutive disparities"""
    multi, first, second = two_minima(S)
    return int((multi & (first // group != second // group)).sum())


def oracle_select(S, W, minD, uniq=10, d12=1):
    from oracle import oracle as orc
    H, _, D = S.shape
    S = np.ascontiguousarray(S, np.uint16)
    raw = np.empty((H, W), np.int16)
    orc.lib().orc_sgm_select(S.ctypes.data_as(C.POINTER(C.c_uint16)), W, H, D, minD, uniq, d12, raw.ctypes.data_as(C.POINTER(C.c_int16)), W)
    return raw


def finish(raw, kw):
    """median and speckle filter of a raw map, as the oracle chains them"""
    from oracle import oracle as orc
    m = orc.median3x3(raw)
    if kw.get("speckleWindowSize", 100) > 0:
        m = orc.filter_speckles(m, (kw["minDisparity"] - 1) * 16, kw.get("speckleWindowSize", 100), 16 * kw.get("speckleRange", 32))
    return m


# ---- partial_sat --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", hc.ALL_D)
@pytest.mark.parametrize("paths", hc.MODES)
def test_partial_sat_saturates_some_costs_of_most_pixels(paths, D):
    kw, fr = case("partial_sat", D, paths)
    for i, (L, R, Cc, S) in enumerate(fr):
        some, nb, every = saturation(S)
        share = valid_share(hr.reference(L, R, paths, kw), D)
        print("partial_sat D %d frame %d paths %d: some %.3f neighbour %.3f every %.3f valid %.3f" % (D, i, paths, some, nb, every, share))
        assert some >= 0.25 and nb >= 0.10 and share >= 0.30 and every <= 0.50, (i, some, nb, every, share)
        assert int(Cc.max()) + kw["P2"] <= SAT                     # an accepted frame


@pytest.mark.parametrize("D", hc.ALL_D)
def test_partial_sat_saturates_every_cost_of_some_pixels(D):
    """the second parameter set, MODE_HH: pixels without a winner that only the "minS >= 32767" rule rejects (uniquenessRatio 0)"""
    kw, fr = case("partial_sat", D, 8, 1)
    assert kw["uniquenessRatio"] == 0
    total = 0
    for i, (L, R, Cc, S) in enumerate(fr):
        every = (S >= SAT).all(2)
        raw = oracle_select(S, L.shape[1], 0, 0)
        print("partial_sat set 1 D %d frame %d: %d pixels with every cost saturated" % (D, i, int(every.sum())))
        total += int(every.sum())
        assert (raw[:, D:][every] == -16).all()                     # no winner there, although index 0 "wins" the scan
        assert valid_share(hr.reference(L, R, 8, kw), D) >= 0.30
    assert total >= 10, total


# ---- at_limit -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", hc.ALL_D)
@pytest.mark.parametrize("paths", hc.MODES)
def test_at_limit_sits_on_the_overflow_boundary(paths, D):
    kw, fr = case("at_limit", D, paths)
    assert kw["P1"] < kw["P2"] <= 32000                             # what rtdm_sgm_create takes
    assert max(int(Cc.max()) for _, _, Cc, _ in fr) + kw["P2"] == SAT
    top = 0
    for i, (L, R, Cc, S) in enumerate(fr):
        share = valid_share(hr.reference(L, R, paths, kw), D)       # accepted
        assert share >= 0.30, (i, share)
        top = max(top, max(int(sgm_hh4_ref.path_costs(Cc, dx, dy, kw["P1"], kw["P2"]).max()) for dx, dy in sgm_hh4_ref.DIRS[paths]))
    assert top == SAT                                               # the packed recurrence at its bound
    refused = 0
    for L, R, _, _ in fr:
        try:
            hr.reference(L, R, paths, dict(kw, P2=kw["P2"] + 1))
        except ValueError:
            refused += 1
    assert refused >= 1                                             # (the frame that holds the largest block cost)


# ---- ties ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("paths", hc.MODES)
@pytest.mark.parametrize("k", (0, 1), ids=("bs1", "bs5"))
@pytest.mark.parametrize("family,D", [(f, D) for f in ("ties", "ties35") for D in hc.ALL_D])
def test_ties_tie(family, D, k, paths):
    kw, fr = case(family, D, paths, k)
    for i, (L, R, Cc, S) in enumerate(fr):
        multi, first, second = two_minima(S)
        assert multi.mean() >= 0.90, (i, float(multi.mean()))
        # the tied minima in different lanes at 2, 4, 8, 16 disparities per lane (period 4 leaves them in one lane of 8)
        for lane in ((2, 4) if family == "ties" else (2, 4, 8, 16)):
            assert apart(S, lane) >= 100, (i, lane, apart(S, lane))
        if family == "ties35" and D in (128, 256, 272):               # in different 16-lane rows: 4 / 8 / 8 disparities per lane
            assert apart(S, 16 * (4 if D == 128 else 8)) > 0, i
        if family == "ties35" and D == 1040:                          # in different waves: 64 lanes of 8
            assert apart(S, 512) > 0, i
        assert (first < second)[multi].all()


# ---- vote_ties ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", hc.ALL_D)
@pytest.mark.parametrize("minD", (0, 3, -5))
@pytest.mark.parametrize("paths", hc.MODES)
def test_vote_ties_are_decided_by_r7_and_show_in_the_map(paths, minD, D):
    kw, fr = case("vote_ties", D, paths, 0, minD)
    for i, (L, R, Cc, S) in enumerate(fr):
        W = L.shape[1]
        u = kw["uniquenessRatio"]
        raw, events = hr.select(S, W, minD, u)
        assert raw.tobytes() == oracle_select(S, W, minD, u).tobytes()   # the restatement IS the oracle's selection
        flipped, _ = hr.select(S, W, minD, u, larger_x_stays=False)
        print("vote_ties D %d frame %d paths %d minD %d: %d events, the other rule changes %d pixels" % (D, i, paths, minD, events, int((raw != flipped).sum())))
        assert events >= 10, (i, events)
        assert (raw != flipped).any(), i
        if minD == 0:
            want = hr.reference(L, R, paths, kw)
            assert want.tobytes() == finish(raw, kw).tobytes()
            assert (finish(flipped, kw) != want).any(), i


# ---- ends, steps --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", hc.ALL_D)
@pytest.mark.parametrize("minD", (0, 3, -5))
@pytest.mark.parametrize("paths", hc.MODES)
def test_ends_put_winners_on_both_ends(paths, minD, D):
    kw, fr = case("ends", D, paths, 0, minD)
    for i, (L, R, Cc, S) in enumerate(fr):
        bd = S.argmin(2)
        lo, hi = float((bd == 0).mean()), float((bd == D - 1).mean())
        assert lo >= 0.15 and hi >= 0.15, (i, lo, hi)
        assert (hr.reference(L, R, paths, kw) != (minD - 1) * 16).sum() >= 0.30 * S.shape[0] * S.shape[1]


@pytest.mark.parametrize("D", hc.ALL_D)
@pytest.mark.parametrize("paths", hc.MODES)
def test_steps_make_disp12maxdiff_live(paths, D):
    kw, fr = case("steps", D, paths)
    for i, (L, R, Cc, S) in enumerate(fr):
        m = {v: hr.reference(L, R, paths, dict(kw, disp12MaxDiff=v)) for v in (-1, 0, 1, 2)}
        assert m[-1].tobytes() == m[0].tobytes() == m[1].tobytes()      # the check is always on
        assert int((m[1] != m[2]).sum()) >= 10, i


@pytest.mark.parametrize("D", hc.ALL_D)
@pytest.mark.parametrize("family", ("ends", "steps", "vote_ties"))
def test_mind_3_makes_the_scaled_invalid_vote_live(family, D):
    """R9 initialises the votes with (minD - 1) * 16, which counts as a vote ">= minD" from minD = 2 on"""
    changed = 0
    for paths in hc.MODES:
        kw, fr = case(family, D, paths, 0, 3)
        for L, R, Cc, S in fr:
            W = L.shape[1]
            u, d12 = kw.get("uniquenessRatio", 10), kw.get("disp12MaxDiff", 1)
            raw, _ = hr.select(S, W, 3, u, d12)
            assert raw.tobytes() == oracle_select(S, W, 3, u, d12).tobytes()
            changed += int((raw != hr.select(S, W, 3, u, d12, scaled_invalid_votes=False)[0]).sum())
    assert changed >= 1


# ---- uniqueness pins ----------------------------------------------------------------------------------------------------------------
def pin_frames(family, D, seed):
    W1, H = hc.shape(D)
    return sh.make(family, seed, hc.width(D, 0, W1), H, D)


@pytest.mark.parametrize("family,D,paths,seed,u", hc.PINS, ids=["%s-D%d-p%d-s%d-u%d" % p for p in hc.PINS])
def test_uniqueness_pins_are_live(family, D, paths, seed, u):
    L, R = pin_frames(family, D, seed)
    kw = hr.resolve(hc.param_sets(family, paths)[0], L[None], R[None], D, 0)
    a = hr.reference(L, R, paths, dict(kw, uniquenessRatio=u))
    b = hr.reference(L, R, paths, dict(kw, uniquenessRatio=u + 1))
    assert (a != b).any()


def test_every_route_shape_has_a_pin():
    assert {(D, p) for _, D, p, _, _ in hc.PINS} >= {(D, p) for D in hc.NARROW_D + hc.WIDE_D for p in hc.MODES}
    assert {f for f, _, _, _, _ in hc.PINS} == {"partial_sat", "vote_ties"}


def test_the_saturated_pin_rejects_through_a_saturated_cost():
    family, D, paths, seed, u = hc.SAT_PIN
    assert hc.SAT_PIN in hc.PINS
    L, R = pin_frames(family, D, seed)
    kw = hr.resolve(hc.param_sets(family, paths)[0], L[None], R[None], D, 0)
    _, S = hr.volumes(L, R, paths, kw)
    S = S.astype(np.int64)
    mins, bd = S.min(2), S.argmin(2)
    far = np.abs(np.arange(D)[None, None, :] - bd[:, :, None]) > 1

    def rejecting(uu):
        return (S * (100 - uu) < (mins * 100)[:, :, None]) & far
    r0, r1 = rejecting(u), rejecting(u + 1)
    fresh = ~r0.any(2) & r1.any(2) & (mins < SAT)                    # accepted at u, rejected at u + 1
    by_saturated = fresh & (~r1 | (S >= SAT)).all(2)                 # ... and only costs at 32767 reject
    assert by_saturated.any()
