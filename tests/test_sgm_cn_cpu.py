"""The colour / preFilterCap generalisation of StereoSGBM's pixel cost (R1) on the CPU side: the NumPy restatement in
sgm_cn_ref.py against the C oracle where the two overlap (gray, ftzero = 15), the ftzero rule, the bound M, and the channel
sum.  The GPU tests (test_gpu_sgm_cn.py) compare against this restatement bit for bit."""
import numpy as np
import pytest

import sgm_cn_ref as ref


def textured(seed, W, H, cn=1, shift=6):
    rng = np.random.default_rng(seed)
    T = rng.integers(0, 256, (H, W + shift, cn)).astype(np.float64)
    T = (T + np.roll(T, 1, 1) + np.roll(T, 1, 0)) / 3
    T = T.astype(np.uint8)
    L, R = T[:, shift:].copy(), T[:, :W].copy()
    return (L[:, :, 0].copy(), R[:, :, 0].copy()) if cn == 1 else (L, R)


@pytest.mark.parametrize("cap", [0, 7, 15])
@pytest.mark.parametrize("minD,D", [(0, 16), (-5, 32), (3, 16)])
def test_gray_pixel_cost_equals_oracle(oracle, cap, minD, D):
    L, R = textured(11 + cap + D, 61, 9)
    pix, _, _ = oracle.sgm_stages(L, R, numDisparities=D, minDisparity=minD, blockSize=3)
    assert np.array_equal(ref.pixel_cost(L, R, minD, D, cap), pix)


@pytest.mark.parametrize("kw", [
    dict(numDisparities=16, minDisparity=0, paths=5),
    dict(numDisparities=16, minDisparity=-7, paths=8, blockSize=3),
    dict(numDisparities=32, minDisparity=4, paths=5, blockSize=7, speckleWindowSize=0),
    dict(numDisparities=16, minDisparity=2, paths=8, blockSize=1, uniquenessRatio=0, disp12MaxDiff=2),
    dict(numDisparities=32, minDisparity=-40, paths=8, blockSize=5),
])
def test_chain_equals_oracle_compute(oracle, kw):
    L, R = textured(100 + kw["numDisparities"] + kw["minDisparity"], 70, 14)
    assert np.array_equal(ref.sgm_compute_cn(L, R, **kw), oracle.sgm_compute(L, R, **kw))


def test_domain_empty_returns_invalid(oracle):
    L, R = textured(5, 40, 6)
    kw = dict(numDisparities=48, minDisparity=0)
    got = ref.sgm_compute_cn(L, R, **kw)
    assert np.array_equal(got, oracle.sgm_compute(L, R, **kw))
    assert (got == -16).all()


def test_refused_frame_matches_oracle(oracle):
    # unrelated binary noise in the two views and a window > 17: the oracle refuses the frame, so must the chain
    rng = np.random.default_rng(1)
    L, R = ((rng.integers(0, 2, (2, 30, 80)) * 255).astype(np.uint8))
    kw = dict(numDisparities=16, blockSize=31, P2=2400, speckleWindowSize=0)
    with pytest.raises(ValueError):
        oracle.sgm_compute(L, R, **kw)
    with pytest.raises(ref.CostOverflow):
        ref.sgm_compute_cn(L, R, **kw)


def test_ftzero_table():
    assert [ref.ftzero(c) for c in (0, 15, 16, 31, 63, 64, 96, 97, 127)] == [15, 15, 17, 31, 63, 65, 97, 97, 127]


def test_max_pixel_cost_corners():
    assert ref.max_pixel_cost(1, 0) == 93
    assert ref.max_pixel_cost(1, 95) == 253            # ftzero 95: the largest that fits the u8 forms (ftzero is odd)
    assert ref.max_pixel_cost(1, 96) == 257            # ftzero 97: the first gray cap that needs u16 pixel costs
    assert ref.max_pixel_cost(3, 0) == 279
    assert ref.max_pixel_cost(3, 127) == 951


@pytest.mark.parametrize("cap", [0, 31, 97, 127])
def test_equal_channels_cost_three_times_gray(cap):
    L, R = textured(31 + cap, 50, 8)
    L3, R3 = np.repeat(L[:, :, None], 3, 2), np.repeat(R[:, :, None], 3, 2)
    for minD, D in ((0, 16), (-3, 32)):
        assert np.array_equal(ref.pixel_cost(L3, R3, minD, D, cap).astype(np.int64),
                              3 * ref.pixel_cost(L, R, minD, D, cap).astype(np.int64))


@pytest.mark.parametrize("cn,cap", [(1, 0), (1, 63), (1, 127), (3, 0), (3, 127)])
def test_pixel_cost_reaches_its_bound(cn, cap):
    # unrelated binary noise in the two views (the same in every channel): some pixel reaches M = cn (2 ftzero + 63), none passes it
    rng = np.random.default_rng(3)
    L, R = (rng.integers(0, 2, (2, 20, 60)) * 255).astype(np.uint8)
    if cn == 3:
        L, R = np.repeat(L[:, :, None], 3, 2), np.repeat(R[:, :, None], 3, 2)
    assert ref.pixel_cost(L, R, 0, 16, cap).max() == ref.max_pixel_cost(cn, cap)


def test_colour_channels_are_summed_independently():
    L, R = textured(77, 48, 7, cn=3)
    total = ref.pixel_cost(L, R, -2, 16, 31).astype(np.int64)
    parts = sum(ref.pixel_cost(L[:, :, c].copy(), R[:, :, c].copy(), -2, 16, 31).astype(np.int64) for c in range(3))
    assert np.array_equal(total, parts)
