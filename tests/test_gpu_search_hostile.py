"""Every route of the StereoBM search stage on pairs that ATTAIN its arithmetic bounds (tests/hostile_pairs.py: worst-case
SADs, ties a period apart, winners on and beside both ends of the range, thresholds hit exactly), bit for bit against the
oracle.  tests/test_hostile_pairs_cpu.py shows on the CPU that the pairs do what they claim and that the thresholds pinned in
tests/hostile_cases.py are live; tests/test_search_plan_cpu.py pins the routes, the largest cap of each and the strip lengths
of the long-strip batches."""
import contextlib
import functools

import numpy as np
import pytest

import hostile_cases as hc
import hostile_pairs as hp
from conftest import load
from test_gpu_dslice import assert_same, forced_slice
from test_gpu_fuzz import FAST_TABLE, RING_TABLE
from test_gpu_search_routes import ROWS

pytestmark = pytest.mark.gpu

N = 16
OFF = dict(uniquenessRatio=0, textureThreshold=0, speckleWindowSize=0, disp12MaxDiff=-1)
ALL_TIES = ("worst", "ties")              # L == R up to a shift of the period: every minimum ties, uniquenessRatio 10 filters all
RING_VARIANT = {2: "fast_ring_qsad", 4: "fast_ring4_qsad", 8: "fast_ring8_qsad", 16: "fast_ring16_qsad"}


@pytest.fixture(scope="module")
def pkg():
    import torch                         # torch first: it brings its own HIP runtime and must initialise before ours
    assert torch.cuda.is_available(), "the -m gpu suite needs an MI355X"
    return load()


@contextlib.contextmanager
def search_kernel(pkg, mode):
    pkg.binding.lib().rtdm_debug_search_kernel(mode)
    try:
        yield
    finally:
        pkg.binding.lib().rtdm_debug_search_kernel(-1)


@functools.lru_cache(maxsize=64)
def frames(family, seed, n, W, H, D, minD, w):
    L, R = hp.make_n(family, seed, n, W, H, D, minD, w)
    L.setflags(write=False); R.setflags(write=False)
    return L, R


def want_map(oracle, row, L, R, kw):
    W, H, D, w, minD, cap, legacy = row[:7]
    oracle.set_legacy_right_clamp(bool(legacy))
    try:
        return oracle.bm_compute(L, R, numDisparities=D, blockSize=w, minDisparity=minD, preFilterCap=cap, nthreads=4, **kw)
    finally:
        oracle.set_legacy_right_clamp(False)


def matcher(pkg, row, n, kw):
    W, H, D, w, minD, cap, legacy = row[:7]
    return pkg.HIPMatcher(numOfDisparities=D, blockSize=w, minDisparity=minD, preFilterCap=cap, width=W, height=H, max_batch=n,
                          legacy_right_clamp=legacy, **kw)


def run(pkg, row, L, R, kw):
    """L, R [n, H, W]: one frame through compute, more through compute_device.  -> (maps [n, H, W], variant)"""
    n = L.shape[0]
    m = matcher(pkg, row, n, kw)
    try:
        if n == 1:
            got = m.compute(L[0], R[0])[None]
        else:
            import torch
            dD = torch.full(L.shape, 12345, dtype=torch.int16, device="cuda")
            m.compute_device(torch.from_numpy(np.array(L)).cuda(), torch.from_numpy(np.array(R)).cuda(), dD, torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            got = dD.cpu().numpy()
        return got, m.search_variant
    finally:
        m.close()


def check(pkg, oracle, row, variant, family, seed, n, kw, valid=True, swap=False):
    """n frames of `family` (frame i: seed + i) at the row's shape; the first and the last against the oracle."""
    W, H, D, w, minD, cap = row[:6]
    L, R = frames(family, seed, n, W, H, D, 0 if swap else minD, w)
    if swap:                                                 # the right matcher's geometry: views swapped, minD = 1 - D
        L, R = R, L
    got, got_variant = run(pkg, row, L, R, kw)
    what = "%s seed %d n=%d %dx%d D=%d w=%d minD=%d cap=%d legacy=%d %s variant=%s" % ((family, seed, n) + tuple(row[:7]) + (kw, got_variant))
    assert got_variant == variant, what
    for i in sorted({0, n - 1}):
        want = want_map(oracle, row, L[i], R[i], kw)
        share = float((want != (minD - 1) * 16).mean())
        print("%s frame %d: %.3f of the oracle's pixels are valid" % (what, i, share))
        assert_same(got[i], want, "%s frame %d" % (what, i))
        if valid:
            assert share > 0.05, what


# ---- 1. the routes ------------------------------------------------------------------------------------------------------
ROUTE_CASES = [(r[:7], r[7]) for r in ROWS] + [(hc.with_cap(r[:7], hc.MAXCAP[r[:7]]), r[7]) for r in ROWS if hc.MAXCAP[r[:7]] != r[5]]
ROUTE_IDS = ["%dx%d-D%d-w%d-minD%d-cap%d-legacy%d" % r for r, _ in ROUTE_CASES]


@pytest.mark.parametrize("n", (1, N))
@pytest.mark.parametrize("row,variant", ROUTE_CASES, ids=ROUTE_IDS)
def test_every_family_on_every_route(pkg, oracle, row, variant, n):
    for k, family in enumerate(hp.FAMILIES):
        check(pkg, oracle, row, variant, family, 100 + k, n, OFF)
        check(pkg, oracle, row, variant, family, 100 + k, n, {}, valid=family not in ALL_TIES)


@pytest.mark.parametrize("n", (1, N))
@pytest.mark.parametrize("row,variant", ROUTE_CASES, ids=ROUTE_IDS)
def test_thresholds_on_their_live_boundaries(pkg, oracle, row, variant, n):
    # (the valid share is not asserted for the textureThreshold pins: several w cap are meant to filter most of a bars frame)
    for name, family, seed, v in hc.PINS[row]:
        for u in ((0, 1, 2) if name == hc.D12 else (v, v + 1)):
            check(pkg, oracle, row, variant, family, seed, n, hc.pin_params(name, u), valid=name != hc.TEX)


# ---- 2. every ring instantiation ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,w,lpp", RING_TABLE)
def test_every_ring_instantiation(pkg, oracle, D, w, lpp):
    with search_kernel(pkg, lpp):
        for cap in (31, hc.largest_ring_cap(w)):
            rc = hc.ring_rows_cap(w, cap)
            W, H = D + 4 * w + 150, w + 7 + 3 * min(rc, 40)
            if hc.ring_rebase_trips(D, w, lpp, cap) == 0:   # no rebasing: at least three strips here (of 12 or 15 - 16 rows: the
                assert -(-(H - (w - 1)) // rc) >= 3          # full allowed length is test_forms_that_do_not_rebase's)
            row = (W, H, D, w, 0, cap, 0)
            for k, family in enumerate(("worst", "worst_noise", "ties", "edges")):
                check(pkg, oracle, row, RING_VARIANT[lpp], family, 20 + k + lpp, 1, OFF)
            for k, family in enumerate(("worst_noise", "edges")):
                check(pkg, oracle, row, RING_VARIANT[lpp], family, 30 + k + lpp, 1, {})


# ---- 3. strips longer than two rebase intervals ---------------------------------------------------------------------------
def long_strips(pkg, oracle, n, row, lpp, family, kw):
    """Four frames of `family` replicated to a batch of n on the device, ONE compute_device call on a fresh handle (the strip
    tuner re-times on the second sighting of a batch shape: the strip count is the model's, which test_search_plan_cpu pins);
    every frame against its source's oracle map, on the device."""
    import torch
    W, H, D, w, minD, cap = row[:6]
    L, R = frames(family, 0, 4, W, H, D, minD, w)            # (seeds 0 .. 3: the saturated indices of every residue mod 4)
    assert n % 4 == 0 and 2 * n * H * W <= 45e6
    dL = torch.from_numpy(np.array(L)).cuda().repeat(n // 4, 1, 1)
    dR = torch.from_numpy(np.array(R)).cuda().repeat(n // 4, 1, 1)
    dD = torch.full((n, H, W), 12345, dtype=torch.int16, device="cuda")
    m = matcher(pkg, row, n, kw)
    try:
        m.compute_device(dL, dR, dD, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        variant = m.search_variant
    finally:
        m.close()
    what = "%s n=%d %s %s variant=%s" % (family, n, row, kw, variant)
    assert variant == RING_VARIANT[lpp], what
    want = np.stack([want_map(oracle, row, L[i], R[i], kw) for i in range(4)])
    assert (want != (minD - 1) * 16).mean() > 0.05, what
    dW = torch.from_numpy(want).cuda().repeat(n // 4, 1, 1)
    bad = (dD != dW).flatten(1).any(1).nonzero().flatten()
    if bad.numel():
        i = int(bad[0])
        assert_same(dD[i].cpu().numpy(), want[i % 4], "%s: %d frames differ, first %d" % (what, bad.numel(), i))


@pytest.mark.parametrize("n,row,lpp", hc.LONG_STRIPS, ids=["lanes%d" % c[2] for c in hc.LONG_STRIPS])
def test_strips_longer_than_two_rebase_intervals(pkg, oracle, n, row, lpp):
    with search_kernel(pkg, lpp):
        long_strips(pkg, oracle, n, row, lpp, "worst", OFF)
        long_strips(pkg, oracle, n, row, lpp, "worst_noise", OFF)


@pytest.mark.parametrize("n,row,lpp", hc.NO_REBASE_STRIPS, ids=["D%d-w%d-lanes%d" % (c[1][2], c[1][3], c[2]) for c in hc.NO_REBASE_STRIPS])
def test_forms_that_do_not_rebase_on_strips_of_the_full_allowed_length(pkg, oracle, n, row, lpp):
    # three strips of exactly ring_rows_cap output rows each (pinned in test_search_plan_cpu): ring_min_strips is all that keeps
    # the packed prefix sums of these forms inside 16 bits, and `worst` makes them grow as fast as they can
    with search_kernel(pkg, lpp):
        long_strips(pkg, oracle, n, row, lpp, "worst", OFF)
        long_strips(pkg, oracle, n, row, lpp, "worst_noise", OFF)


# ---- 4. k_search_fast ---------------------------------------------------------------------------------------------------------
FAST_CASES = [(D, p) for D, p in FAST_TABLE if D in (64, 80)]     # one D per piece count 2 .. 6 and tail length (1: D 80, 3: D 64)


@pytest.mark.parametrize("D,pieces", FAST_CASES)
def test_fast_instantiations_at_their_largest_cap(pkg, oracle, D, pieces):
    w = 4 * (pieces - 1) + (1 if (D // 16 + pieces) % 2 else 3)
    cap = max(c for c in range(1, 64) if 2 * c * w * w <= 32766)
    row = (D + 4 * w + 150, w + 37, D, w, 0, cap, 0)
    with search_kernel(pkg, 0):
        for k, family in enumerate(("worst", "ties")):
            for seed in (40 + k, 41 + k):
                check(pkg, oracle, row, "fast_qsad", family, seed, 1, OFF)
            check(pkg, oracle, row, "fast_qsad", family, 40 + k, 1, {}, valid=False)


# ---- 5. border kernels ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (1, N))
@pytest.mark.parametrize("row,variant", [(hc.BORDER_ROWS_ROW, "fast_ring4_qsad"), (hc.BORDER_DISP_ROW, "fast_qsad")], ids=("rows", "disp"))
def test_border_columns_at_their_bounds(pkg, oracle, row, variant, n):
    # (the border columns lie outside the valid rectangle; they reach the map through the left-right check: disp12MaxDiff 0, 1)
    assert row[1] >= 64 + row[3] + 8
    for k, family in enumerate(("worst", "ties", "worst_noise", "edges")):
        check(pkg, oracle, row, variant, family, 50 + k, n, OFF)
        check(pkg, oracle, row, variant, family, 50 + k, n, dict(uniquenessRatio=0, textureThreshold=0, speckleWindowSize=0, disp12MaxDiff=0))
        check(pkg, oracle, row, variant, family, 50 + k, n, dict(speckleWindowSize=0), valid=family not in ALL_TIES)


# ---- 6. generic and sliced --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap,variant", [(52, "generic_u16"), (53, "generic_u32")])
def test_generic_kernels_on_either_side_of_16_bits(pkg, oracle, cap, variant):
    w = 25
    assert 2 * cap * w * w < 65536 if variant == "generic_u16" else 2 * (cap - 1) * w * w < 65536 <= 2 * cap * w * w
    row = (300, 90, 64, w, 0, cap, 0)
    for k, family in enumerate(hp.FAMILIES):
        check(pkg, oracle, row, variant, family, 60 + k, 1, OFF)
        check(pkg, oracle, row, variant, family, 60 + k, 1, {}, valid=family not in ALL_TIES)


@pytest.mark.parametrize("dt", (16, 32, 48))
@pytest.mark.parametrize("row", [ROWS[0][:7], ROWS[9][:7]], ids=("D64", "D272"))
def test_forced_slices(pkg, oracle, row, dt):
    # ties a period apart straddle the slice edges (periods 3 and 5 divide no slice width); the range ends sit in the first
    # and in the last slice
    with forced_slice(pkg, dt):
        for family in ("ties", "edges"):
            for seed in (70, 71, 72):
                check(pkg, oracle, row, "generic_dslice_u16", family, seed, 1, OFF)
            check(pkg, oracle, row, "generic_dslice_u16", family, 70, 1, {}, valid=family not in ALL_TIES)


# ---- 7. the right matcher's geometry ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (1, N))
def test_right_matcher_geometry(pkg, oracle, n):
    row = (300, 80, 64, 9, 1 - 64, 31, 0)
    for k, family in enumerate(("edges", "worst", "worst_noise")):
        check(pkg, oracle, row, "fast_ring4_qsad", family, 80 + k, n, OFF, swap=True)
