"""The paired layout of k_search_ring<64, 9, 4> (two adjacent columns per lane, k_search_ring.hip: RingCfg::PAIR) against the
oracle, bit for bit, at the smallest shapes where pairing can go wrong: a pair with one live column, an odd interior, a tile edge
inside and between pairs, partial row groups and a window that is still filling, a setROI1 edge between the two columns of a
pair, ties on plateaus, waves whose selection is skipped, strips longer than the rebase interval, and both instantiations (the
border workgroups in the grid: batch 1; tile-only: batches of 16 and 17)."""
import numpy as np
import pytest

import hostile_pairs
from conftest import load

pytestmark = pytest.mark.gpu

D, WS = 64, 9
WIDTHS = (72, 73, 74, 134, 135, 136, 137)      # interior = W - 71 columns: 1, 2, 3 and 63 .. 66 (a tile is 64)
HEIGHTS = (10, 11, 12, 13, 17)                 # valid rows H - 8: 2 .. 5 and 9 (rows go in groups of four; the window fills for 8)
# ONE valid row: a frame of 9 rows is refused like cv::StereoBM refuses it (blockSize >= height), so the search gets its single
# row from a frame of 10 rows whose setROI1 rectangle is 9 rows high (the valid rectangle loses 4 rows at either end)
ONE_ROW = (10, 9)
HOSTILE_OFF = dict(uniquenessRatio=0, textureThreshold=0, speckleWindowSize=0, disp12MaxDiff=-1)
HIGH_TEX = 600                                 # noise sums to ~2000 per window, a plateau to 0: plateau waves skip the selection


@pytest.fixture(scope="module")
def pkg():
    import torch
    assert torch.cuda.is_available()
    return load()


def _noise(seed, W, H, n=1):
    return hostile_pairs.noise_bands(seed, W, H, D, n)


def _plateaus(seed, W, H, n=1):
    # constant blocks in both views: zero texture, and every SAD inside them ties (the FIRST minimum has to win)
    return hostile_pairs.plateau_noise_n(seed, W, H, D, n)


def _synth(seed, W, H, n=1):
    s = load("synth")
    L, R = s.make_stream(seed, n, W, H, D)
    return np.ascontiguousarray(L), np.ascontiguousarray(R)


CONTENT = {"noise": _noise, "plateaus": _plateaus, "synth": _synth}


def _run(pkg, L, R, roi1=None, **kw):
    """All frames of L, R ([n, H, W]) through one handle; batch 1 through the host path, larger ones as device tensors."""
    n, H, W = L.shape
    m = pkg.HIPMatcher(numOfDisparities=D, blockSize=WS, width=W, height=H, max_batch=n, **kw)
    if roi1: m.setROI1(roi1)
    if n == 1:
        got = m.compute(L[0], R[0])[None]
    else:
        import torch
        dD = torch.full((n, H, W), 12345, dtype=torch.int16, device="cuda")
        m.compute_device(torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda(), dD, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        got = dD.cpu().numpy()
    assert m.search_variant == "fast_ring4_qsad", m.search_variant
    m.close()
    return got


def _check(pkg, oracle, L, R, frames=None, roi1=None, period=0, **kw):
    """frames: the ones compared with the oracle (None: all).  period > 0: frame i is a copy of frame i % period, and every
    frame's map must equal that of its source -- with the first `period` frames among `frames`, every frame is checked."""
    got = _run(pkg, L, R, roi1=roi1, **kw)
    for i in range(period, L.shape[0] if period else 0):
        assert np.array_equal(L[i], L[i % period]) and np.array_equal(R[i], R[i % period])
        assert np.array_equal(got[i], got[i % period]), "frame %d differs from frame %d, which has the same input" % (i, i % period)
    for i in (range(L.shape[0]) if frames is None else frames):
        want = oracle.bm_compute(L[i], R[i], numDisparities=D, blockSize=WS, roi1=roi1, **kw)
        if not np.array_equal(got[i], want):
            bad = np.argwhere(got[i] != want)
            raise AssertionError("%dx%d frame %d %s roi1=%s: %d pixels differ, first (y, x) = %s got %d want %d" % (
                L.shape[2], L.shape[1], i, kw, roi1, len(bad), tuple(bad[0]), got[i][tuple(bad[0])], want[tuple(bad[0])]))


@pytest.mark.parametrize("content", sorted(CONTENT))
@pytest.mark.parametrize("W", WIDTHS)
def test_every_width_and_height(pkg, oracle, content, W):
    for H in HEIGHTS:
        L, R = CONTENT[content](100 * W + H, W, H)
        _check(pkg, oracle, L, R)
    L, R = CONTENT[content](100 * W, W, ONE_ROW[0])
    _check(pkg, oracle, L, R, roi1=(0, 0, W, ONE_ROW[1]))


@pytest.mark.parametrize("cap", (31, 63))
@pytest.mark.parametrize("tex", (0, HIGH_TEX))
@pytest.mark.parametrize("uniq", (0, 15))
@pytest.mark.parametrize("minD", (-7, 5))
def test_parameters(pkg, oracle, cap, tex, uniq, minD):
    # (a minDisparity of either sign costs the interior |minDisparity| columns and more: 12 columns on top of the widths above)
    for k, (W, H) in enumerate(((137 + 12, 31), (74 + 12, 12), (202 + 12, 22))):
        L, R = _plateaus(7000 + 8 * cap + tex + uniq + minD + k, W, H)
        _check(pkg, oracle, L, R, preFilterCap=cap, textureThreshold=tex, uniquenessRatio=uniq, minDisparity=minD)


@pytest.mark.parametrize("n", (16, 17))
@pytest.mark.parametrize("content", sorted(CONTENT))
def test_batches_run_the_tile_only_instantiation(pkg, oracle, content, n):
    # three distinct frames, repeated: the first three (and the last) against the oracle, every other one against its source
    rep = np.arange(n) % 3
    for W, H in ((73, 10), (135, 13), (137, 17), (200, 40)):
        L, R = CONTENT[content](300 * n + W, W, H, 3)
        _check(pkg, oracle, np.ascontiguousarray(L[rep]), np.ascontiguousarray(R[rep]), frames=(0, 1, 2, n - 1), period=3)
    L, R = _plateaus(17 + n, 136, 30, 3)
    _check(pkg, oracle, np.ascontiguousarray(L[rep]), np.ascontiguousarray(R[rep]), frames=(0, 1, 2, n - 1), period=3,
           preFilterCap=63, textureThreshold=HIGH_TEX, uniquenessRatio=15, minDisparity=-7)


@pytest.mark.parametrize("n", (1, 16))
def test_roi_edge_between_the_columns_of_a_pair(pkg, oracle, n):
    # the valid rectangle is the ROI less four columns and rows at either side: 4-5 and 2 columns wide here.  Four consecutive
    # left edges, right edges of both parities: whatever the pairs' parity, some fall between the columns of a pair
    W, H = 210, 26
    L, R = _plateaus(4100 + n, W, H, min(n, 2))
    rep = np.arange(n) % 2 if n > 1 else np.zeros(1, int)
    L, R = np.ascontiguousarray(L[rep]), np.ascontiguousarray(R[rep])
    fr, per = ((0, 1, n - 1), 2) if n > 1 else ((0,), 0)
    for k in range(4):
        _check(pkg, oracle, L, R, frames=fr, period=per, roi1=(96 + k, 5, 12 + k // 2, 14))
        _check(pkg, oracle, L, R, frames=fr, period=per, roi1=(131 + k, 2, 10, 20), uniquenessRatio=0)


@pytest.mark.parametrize("n", (1, 16))
@pytest.mark.parametrize("minD", (-63, -64, -100))
def test_left_copy_starts_in_front_of_the_row(pkg, oracle, minD, n):
    # minDisparity <= 1 - D (what createRightMatcher sets): the left plane is read from its first column on, and the first
    # tile's copy starts three bytes in front of the row -- in frame 0, row 0 in front of the plane itself
    for W, H in ((140, 12), (203, 21)):
        L, R = _plateaus(6000 - minD + n, W, H, min(n, 2))
        rep = np.arange(n) % 2 if n > 1 else np.zeros(1, int)
        _check(pkg, oracle, np.ascontiguousarray(R[rep]), np.ascontiguousarray(L[rep]), frames=(0, 1, n - 1) if n > 1 else (0,),
               period=2 if n > 1 else 0, minDisparity=minD, textureThreshold=0, uniquenessRatio=0)


@pytest.mark.parametrize("cap", (31, 63))
def test_one_frame_of_200_rows(pkg, oracle, cap):
    for content in sorted(CONTENT):
        L, R = CONTENT[content](5000 + cap, 150, 208)
        _check(pkg, oracle, L, R, preFilterCap=cap)


@pytest.mark.parametrize("cap", (31, 63))
def test_strips_longer_than_the_rebase_interval(pkg, oracle, cap):
    # Long strips come with many workgroups only (ring_strips_model: strips ~ sqrt(rows x workgroups in flight / (4 x tiles x
    # frames))): 8192 frames of one tile and 192 valid rows are cut into two strips of 96 rows, which walk 104 rows -- at cap
    # 63 the ring is rebased every 40 rows (65535 / (9 x 126) - 15 = 42 rows, two trips of 20), so a strip crosses two
    # rebases of both rings; at cap 31 (100 rows) one.  The frames are copies of four: every frame must be its source's map.
    import torch
    n, W, H = 8192, 128, 200
    # (plateaus; then the two families of tests/hostile_pairs.py whose window sums attain 2 cap w w -- the prefix sums grow as
    # fast as the rebase interval allows -- with every threshold off, or uniqueness would filter their tied minima)
    for content, kw in (("plateaus", {}), ("worst", HOSTILE_OFF), ("worst_noise", HOSTILE_OFF)):
        L, R = _plateaus(900 + cap, W, H, 4) if content == "plateaus" else hostile_pairs.make_n(content, 0, 4, W, H, D, 0, WS)
        dL = torch.from_numpy(L).cuda().repeat(n // 4, 1, 1)
        dR = torch.from_numpy(R).cuda().repeat(n // 4, 1, 1)
        dD = torch.full((n, H, W), 12345, dtype=torch.int16, device="cuda")
        m = pkg.HIPMatcher(numOfDisparities=D, blockSize=WS, preFilterCap=cap, width=W, height=H, max_batch=n, **kw)
        m.compute_device(dL, dR, dD, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert m.search_variant == "fast_ring4_qsad"
        m.close()
        want = np.stack([oracle.bm_compute(L[i], R[i], numDisparities=D, blockSize=WS, preFilterCap=cap, **kw) for i in range(4)])
        dW = torch.from_numpy(want).cuda().repeat(n // 4, 1, 1)
        bad = (dD != dW).flatten(1).any(1).nonzero().flatten()
        assert bad.numel() == 0, "%s cap %d: %d frames differ, first %d" % (content, cap, bad.numel(), int(bad[0]))
        del dL, dR, dD, dW
