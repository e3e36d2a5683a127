"""The texture window sums of the paired ring search k_search_ring<64, 9, 4> (one row term per owner lane and row group, a u16
prefix ring per column: k_search_ring.hip, RingTexture) against the oracle, bit for bit: every residue of the row count below
and above one trip of the row loop, thresholds that filter part of a frame, thresholds on their live boundaries, and strips
long enough that the 16-bit prefix wraps.  tests/test_ring_texture_cpu.py restates the bookkeeping on the CPU and pins the strip
length of the wrap batch.  Both instantiations: the border workgroups in the grid (n = 1) and tile-only (n = 16)."""
import numpy as np
import pytest

import hostile_cases as hc
import hostile_pairs as hp
from conftest import load
from test_ring_texture_cpu import WRAP_BATCH

pytestmark = pytest.mark.gpu

D, WS = 64, 9
VARIANT = "fast_ring4_qsad"
HEIGHTS = (17, 18, 19, 20, 61, 62, 63, 64)     # valid rows H - 8: 9 .. 12 and 53 .. 56 -- every residue, below and above one trip of 20
# about the median window sum of prefiltered noise, which saturates most bytes: 77 and 74 of 81 cap (found by sweeping the oracle;
# asserted below: part of the frame is filtered)
NOISE_TEX = {31: 2400, 63: 4680}


@pytest.fixture(scope="module")
def pkg():
    import torch
    assert torch.cuda.is_available(), "the -m gpu suite needs an MI355X"
    return load()


def run(pkg, L, R, **kw):
    """L, R [n, H, W] through one handle: one frame through compute, more through one compute_device call"""
    n, H, W = L.shape
    m = pkg.HIPMatcher(numOfDisparities=D, blockSize=WS, width=W, height=H, max_batch=n, **kw)
    try:
        if n == 1:
            got = m.compute(L[0], R[0])[None]
        else:
            import torch
            dD = torch.full((n, H, W), 12345, dtype=torch.int16, device="cuda")
            m.compute_device(torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda(), dD, torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            got = dD.cpu().numpy()
        assert m.search_variant == VARIANT, m.search_variant
        return got
    finally:
        m.close()


def same(got, want, what):
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError("%s: %d pixels differ, first (y, x) = %s got %d want %d" % (what, len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])]))


def check(pkg, oracle, L2, R2, n, what, part=False, **kw):
    """Two distinct frames, repeated to a batch of n: frames 0, 1 and the last against the oracle, every frame against its source.
    part: -> (pixels the threshold filters of those the oracle finds without it, their number), over the two frames."""
    rep = np.arange(n) % 2
    L, R = np.ascontiguousarray(L2[rep]), np.ascontiguousarray(R2[rep])
    got = run(pkg, L, R, **kw)
    for i in range(2, n):
        same(got[i], got[i % 2], "%s n=%d: frame %d against frame %d, which has the same input" % (what, n, i, i % 2))
    lost = np.zeros(2, int)
    for i in range(min(n, 2)):
        want = oracle.bm_compute(L[i], R[i], numDisparities=D, blockSize=WS, **kw)
        same(got[i], want, "%s n=%d %s frame %d" % (what, n, kw, i))
        if part:
            free = oracle.bm_compute(L[i], R[i], numDisparities=D, blockSize=WS, **dict(kw, textureThreshold=0))
            filt = -16                                       # (minDisparity - 1) * 16
            lost += (int(((free != filt) & (want == filt)).sum()), int((free != filt).sum()))
    return tuple(lost)


def filters_part(lost):
    return any(20 <= a <= b - 20 for a, b in lost)


@pytest.mark.parametrize("n", (1, 16))
@pytest.mark.parametrize("H", HEIGHTS)
def test_row_counts(pkg, oracle, H, n):
    W = 128
    L, R = hp.noise_bands(40 * H + n, W, H, D, 2)
    lost = [check(pkg, oracle, L, R, n, "noise 128x%d" % H, part=True, speckleWindowSize=0, textureThreshold=NOISE_TEX[31] + k * 31) for k in range(2)]
    assert filters_part(lost), "no threshold filters part of the frame: %s" % (lost,)
    L, R = hp.plateau_noise_n(41 * H + n, W, H, D, 2)
    check(pkg, oracle, L, R, n, "plateaus 128x%d" % H)


@pytest.mark.parametrize("n", (1, 16))
@pytest.mark.parametrize("cap", (31, 63))
def test_noise_with_a_threshold_that_filters_part_of_the_frame(pkg, oracle, cap, n):
    for W, H in ((137, 31), (200, 45)):
        L, R = hp.noise_bands(900 + cap + n + W, W, H, D, 2)
        lost = [check(pkg, oracle, L, R, n, "noise %dx%d" % (W, H), part=True, preFilterCap=cap, textureThreshold=tex, speckleWindowSize=0)
                for tex in (NOISE_TEX[cap], NOISE_TEX[cap] + cap)]
        assert filters_part(lost), "no threshold filters part of the frame: %s" % (lost,)
        print("noise %dx%d cap %d: filtered of valid %s" % (W, H, cap, lost))
        check(pkg, oracle, L, R, n, "noise %dx%d" % (W, H), preFilterCap=cap, textureThreshold=NOISE_TEX[cap])   # (speckle filter on)


BAR_ROWS = [row for row in hc.PINS if row[2:5] == (D, WS, 0) and not row[6]]       # the (64, 9) rows at minDisparity 0: cap 31, 56, 63


@pytest.mark.parametrize("n", (1, 16))
@pytest.mark.parametrize("row", BAR_ROWS, ids=["cap%d" % r[5] for r in BAR_ROWS])
def test_bars_on_the_live_texture_boundaries(pkg, oracle, row, n):
    # the pairs k cap | k cap + 1 that tests/test_hostile_pairs_cpu.py shows to be decisive (hostile_cases.PINS)
    W, H, _, _, minD, cap = row[:6]
    pins = [(family, seed, v) for name, family, seed, v in hc.PINS[row] if name == hc.TEX]
    assert len(pins) == 2 and all(f == "bars" and v % cap == 0 for f, _, v in pins)
    for family, seed, v in pins:
        L, R = hp.make_n(family, seed, 2, W, H, D, minD, WS)
        for tex in (v, v + 1):
            check(pkg, oracle, L, R, n, "bars seed %d %dx%d" % (seed, W, H), preFilterCap=cap, **hc.pin_params(hc.TEX, tex))


@pytest.mark.parametrize("tex", (81 * 63, 81 * 63 + 1))
def test_prefix_wraps_16_bits(pkg, oracle, tex):
    # 8192 frames of 80 x 400 are cut into three strips of 131 output rows (test_ring_texture_cpu pins that), which walk 139 rows;
    # in a `worst` frame every prefiltered byte is 0 or 2 cap, every row term 9 x 63, and the 16-bit prefix wraps past row 115.
    # Every window sum is 81 x 63 = 5103: a threshold of 5103 keeps the pixels, 5104 filters every one.  One compute_device call
    # per handle, so the strip model stays in charge.  The frames are copies of four.
    import torch
    n, (W, H, _, _, minD, cap, _) = WRAP_BATCH
    kw = dict(preFilterCap=cap, uniquenessRatio=0, speckleWindowSize=0, disp12MaxDiff=-1, textureThreshold=tex)
    L, R = hp.make_n("worst", 0, 4, W, H, D, minD, WS)
    want = np.stack([oracle.bm_compute(L[i], R[i], numDisparities=D, blockSize=WS, **kw) for i in range(4)])
    # the rectangle the search covers, less its last column: that one's window holds the frame's last column, which the
    # prefilter leaves at cap (no texture), so its sum is 72 cap
    valid = want[:, 4:H - 4, D - 1 + 4:W - 5]
    if tex == 81 * cap:
        assert (valid != -16).all(), "the oracle filters pixels at the threshold itself"
    else:
        assert (want == -16).all(), "the oracle keeps pixels one above the largest window sum"
    dL = torch.from_numpy(L).cuda().repeat(n // 4, 1, 1)
    dR = torch.from_numpy(R).cuda().repeat(n // 4, 1, 1)
    dD = torch.full((n, H, W), 12345, dtype=torch.int16, device="cuda")
    m = pkg.HIPMatcher(numOfDisparities=D, blockSize=WS, width=W, height=H, max_batch=n, **kw)
    try:
        m.compute_device(dL, dR, dD, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert m.search_variant == VARIANT
    finally:
        m.close()
    got4 = dD[:4].cpu().numpy()
    for i in range(4):                                       # the distinct frames against the oracle
        same(got4[i], want[i], "worst frame %d at textureThreshold %d" % (i, tex))
    bad = (dD != dD[:4].repeat(n // 4, 1, 1)).flatten(1).any(1).nonzero().flatten()   # every copy against its source
    assert bad.numel() == 0, "textureThreshold %d: %d frames differ from their source, first %d" % (tex, bad.numel(), int(bad[0]))
