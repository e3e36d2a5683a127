"""StereoBM configurations the generic search kernel cannot hold in LDS -- numDisparities > 256, large windows at large D --
run on the disparity-sliced search kernel (k_search_dslice in k_search_generic.hip).  Every result is compared bit for bit
with the oracle.
rtdm_debug_disparity_slice forces the sliced kernel with a given slice width on any configuration, so that slice
boundaries can be put anywhere; it is reset in `finally` everywhere."""
import contextlib

import numpy as np
import pytest

from conftest import load

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    import torch                         # torch first: it brings its own HIP runtime and must initialise before ours
    assert torch.cuda.is_available(), "the -m gpu suite needs an MI355X"
    return load()


@contextlib.contextmanager
def forced_slice(pkg, dt):
    pkg.binding.lib().rtdm_debug_disparity_slice(dt)
    try:
        yield
    finally:
        pkg.binding.lib().rtdm_debug_disparity_slice(0)


def assert_same(got, want, what=""):
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError("%s: %d / %d pixels differ; first at (y,x)=%s got %d want %d" % (
            what, len(bad), got.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])]))


def hip_kw(kw):
    kw = dict(kw)
    kw["numOfDisparities"] = kw.pop("numDisparities")
    return kw


def run(pkg, oracle, L, R, roi1=None, roi2=None, legacy=0, **kw):
    """-> (device result, oracle result, variant string)"""
    H, W = L.shape
    m = pkg.HIPMatcher(width=W, height=H, legacy_right_clamp=legacy, **hip_kw(kw))
    if roi1: m.setROI1(roi1)
    if roi2: m.setROI2(roi2)
    got = m.compute(L, R)
    variant = m.search_variant
    m.close()
    if legacy:
        oracle.set_legacy_right_clamp(True)
    try:
        want = oracle.bm_compute(L, R, roi1=roi1, roi2=roi2, nthreads=8, **kw)
    finally:
        if legacy:
            oracle.set_legacy_right_clamp(False)
    return got, want, variant


# ---- 1. numDisparities > 256 at the reference's parameters (blockSize 13, cap 31) ------------------------------------
@pytest.mark.parametrize("D,H", [(272, 60), (320, 100), (512, 80), (1024, 64)])
def test_more_than_256_disparities(pkg, oracle, synth, D, H):
    W = D + 300
    L, R = synth.make_pair(synth.STREAM_SEED + 7000 + D, W, H, D)
    got, want, variant = run(pkg, oracle, L, R, numDisparities=D, blockSize=13, preFilterCap=31)
    assert variant.startswith("generic_dslice"), variant
    assert_same(got, want, "D=%d" % D)
    assert (want != -16).mean() > 0.05


# ---- 2. extremes of numDisparities / minDisparity ---------------------------------------------------------------------
@pytest.mark.parametrize("D,minD,W,H", [(2048, -1024, 2348, 40), (4080, -2033, 4096, 30), (512, 300, 1400, 48),
                                        (320, -2047, 2200, 48)])
def test_extreme_disparity_ranges(pkg, oracle, synth, D, minD, W, H):
    L, R = synth.make_pair(synth.STREAM_SEED + 7100 + D + minD, W, H, min(D, 256))
    got, want, variant = run(pkg, oracle, L, R, numDisparities=D, blockSize=13, minDisparity=minD)
    assert variant.startswith("generic_dslice"), variant
    assert_same(got, want, "D=%d minD=%d" % (D, minD))
    if minD == -2047:
        assert want.min() == -32768


# ---- 3. D <= 256 with windows whose column sums did not fit the generic kernel's LDS ---------------------------------
@pytest.mark.parametrize("D,w,cap", [(256, 33, 31), (256, 29, 63), (192, 81, 31), (128, 183, 31)])
def test_large_windows_formerly_refused(pkg, oracle, synth, D, w, cap):
    W, H = D + w + 120, w + 40
    L, R = synth.make_pair(synth.STREAM_SEED + 7200 + D + w, W, H, D)
    got, want, variant = run(pkg, oracle, L, R, numDisparities=D, blockSize=w, preFilterCap=cap)
    assert variant == ("generic_dslice_u16" if 2 * cap * w * w < 65536 else "generic_dslice_u32"), variant
    assert_same(got, want, "D=%d w=%d cap=%d" % (D, w, cap))


# ---- 4. forced slice boundaries on random configurations ---------------------------------------------------------------
def _case(rng):
    D = int(rng.choice([32, 48, 64, 96, 128, 192, 256, 272, 320, 512]))
    w = int(rng.choice([5, 7, 9, 11, 13, 15, 21, 25]))
    minD = int(rng.choice([0, 0, 3, -7, -20, 17]))
    W = int(rng.integers(D + abs(minD) + w + 20, D + abs(minD) + w + 200))
    H = int(rng.integers(w + 3, w + 50))
    kw = dict(numDisparities=D, blockSize=w, minDisparity=minD,
              preFilterCap=int(rng.choice([31, 31, 15, 63, 5])),
              textureThreshold=int(rng.choice([0, 10])),
              uniquenessRatio=int(rng.choice([0, 10, 50])),
              speckleWindowSize=int(rng.choice([100, 0, 20])),
              speckleRange=int(rng.choice([32, 4, 64])),
              disp12MaxDiff=int(rng.choice([-1, 0, 1])))
    roi1 = roi2 = None
    if rng.random() < 0.35:
        x0, y0 = int(rng.integers(0, W // 2)), int(rng.integers(0, H // 2))
        roi1 = (x0, y0, int(rng.integers(1, W - x0 + 1)), int(rng.integers(1, H - y0 + 1)))
    if rng.random() < 0.15:
        x0, y0 = int(rng.integers(0, W // 3)), int(rng.integers(0, H // 3))
        roi2 = (x0, y0, int(rng.integers(W // 2, W - x0 + 1)), int(rng.integers(H // 2, H - y0 + 1)))
    legacy = int(rng.random() < 0.25)
    return W, H, kw, roi1, roi2, legacy


@pytest.mark.parametrize("dt,seeds", [(16, range(48)), (32, range(100, 116)), (48, range(200, 216))])
def test_forced_slices_on_random_configurations(pkg, oracle, synth, dt, seeds):
    with forced_slice(pkg, dt):
        for seed in seeds:
            rng = np.random.default_rng(3000 + seed)
            W, H, kw, roi1, roi2, legacy = _case(rng)
            L, R = synth.make_pair(synth.STREAM_SEED + 6000 + seed, W, H, kw["numDisparities"])
            if seed % 5 == 0:                       # pitched, odd-aligned views
                pad = np.zeros((H + 3, W + 37), np.uint8)
                pl, pr = pad.copy(), pad.copy()
                pl[2:2 + H, 5:5 + W] = L; pr[2:2 + H, 5:5 + W] = R
                L, R = pl[2:2 + H, 5:5 + W], pr[2:2 + H, 5:5 + W]
            got, want, variant = run(pkg, oracle, L, R, roi1=roi1, roi2=roi2, legacy=legacy, **kw)
            # (an ROI can leave no valid pixel: the frame is filled and no search runs)
            assert variant.startswith("generic_dslice") or (want == (kw["minDisparity"] - 1) * 16).all(), variant
            assert_same(got, want, "dt=%d seed=%d %dx%d %s roi1=%s roi2=%s legacy=%d" % (dt, seed, W, H, kw, roi1, roi2, legacy))


# ---- 5. ties and winners on slice edges (texture 0; forced DT = 16 and the library's own slice width) ------------------
EDGE_DT = [16, 0]


def _edge_kw(D, minD, uniq):
    return dict(numDisparities=D, blockSize=9, minDisparity=minD, textureThreshold=0, uniquenessRatio=uniq,
                speckleWindowSize=0, disp12MaxDiff=-1)


@pytest.mark.parametrize("dt", EDGE_DT)
@pytest.mark.parametrize("uniq", [0, 10])
@pytest.mark.parametrize("minD", [0, 1, -1])
def test_periodic_texture_ties_at_every_slice_edge(pkg, oracle, dt, uniq, minD):
    # period 16 divides every slice width: equal minima recur at each slice boundary (+- minD), only "first minimum" decides
    D, W, H = 320, 560, 40
    rng = np.random.default_rng(11 + minD)
    row = rng.integers(0, 256, 16).astype(np.uint8)
    L = np.ascontiguousarray(np.tile(row, (H, W // 16 + 1))[:, :W])
    R = L.copy()
    with forced_slice(pkg, dt):
        got, want, variant = run(pkg, oracle, L, R, **_edge_kw(D, minD, uniq))
    assert variant.startswith("generic_dslice"), variant
    assert_same(got, want, "periodic dt=%d uniq=%d minD=%d" % (dt, uniq, minD))
    if uniq == 0:
        assert (want != (minD - 1) * 16).any()


@pytest.mark.parametrize("dt", EDGE_DT)
@pytest.mark.parametrize("uniq", [0, 10])
@pytest.mark.parametrize("value", [0, 77, 255])
def test_constant_images(pkg, oracle, dt, uniq, value):
    D, W, H = 288, 400, 30
    L = np.full((H, W), value, np.uint8)
    with forced_slice(pkg, dt):
        got, want, variant = run(pkg, oracle, L, L.copy(), **_edge_kw(D, 0, uniq))
    assert variant.startswith("generic_dslice"), variant
    assert_same(got, want, "constant %d dt=%d uniq=%d" % (value, dt, uniq))


@pytest.mark.parametrize("dt", [16, 32, 0])
@pytest.mark.parametrize("uniq", [0, 10])
def test_true_shift_on_slice_edges(pkg, oracle, dt, uniq):
    D, minD, W, H = 320, -5, 640, 36
    slice_w = dt or 16                    # (the library's width is a multiple of 16 too)
    rng = np.random.default_rng(5 + dt)
    base = rng.integers(0, 256, (H, W + D + 8)).astype(np.uint8)
    with forced_slice(pkg, dt):
        for e in sorted({0, D - 1, slice_w - 1, slice_w, slice_w + 1, 2 * slice_w - 1, 2 * slice_w}):
            d = D - 1 + minD - e                                 # reversed index e <-> disparity d
            L = np.ascontiguousarray(base[:, 4:4 + W])
            R = np.ascontiguousarray(base[:, 4 + d:4 + d + W]) if d >= 0 else np.ascontiguousarray(
                np.pad(base, ((0, 0), (-d, 0)))[:, 4:4 + W])
            got, want, variant = run(pkg, oracle, L, R, **_edge_kw(D, minD, uniq))
            assert variant.startswith("generic_dslice"), variant
            assert_same(got, want, "shift e=%d dt=%d uniq=%d" % (e, dt, uniq))
            if uniq == 0:                                        # the shift is found where every shift is searchable
                assert (np.abs(((want[H // 2, 580:620].astype(int) + 8) >> 4) - d) <= 1).mean() > 0.5, (e, d)


# ---- 6. every entry point on the new path, D = 320 ----------------------------------------------------------------------
D6, W6, H6 = 320, 640, 72
KW6 = dict(numDisparities=D6, blockSize=13)


def test_compute_with_pitched_views(pkg, oracle, synth):
    L, R = synth.make_pair(synth.STREAM_SEED + 7300, W6, H6, D6)
    pad = np.zeros((H6 + 5, W6 + 51), np.uint8)
    pl, pr = pad.copy(), pad.copy()
    pl[3:3 + H6, 7:7 + W6] = L; pr[3:3 + H6, 7:7 + W6] = R
    Lv, Rv = pl[3:3 + H6, 7:7 + W6], pr[3:3 + H6, 7:7 + W6]
    m = pkg.HIPMatcher(width=W6, height=H6, **hip_kw(KW6))
    outp = np.full((H6 + 2, W6 + 9), 999, np.int16)
    out = outp[1:1 + H6, 3:3 + W6]
    m.compute(Lv, Rv, out)
    assert m.search_variant.startswith("generic_dslice")
    m.close()
    assert_same(np.ascontiguousarray(out), oracle.bm_compute(L, R, **KW6))
    assert (outp[0] == 999).all() and (outp[:, :3] == 999).all() and (outp[:, 3 + W6:] == 999).all()


def test_compute_device_batch_on_a_torch_stream(pkg, oracle, synth):
    import torch
    n = 3
    Ls, Rs = synth.make_stream(7400, n, W6, H6, D6)
    dL, dR = torch.from_numpy(Ls).cuda(), torch.from_numpy(Rs).cuda()
    dD = torch.zeros((n, H6, W6), dtype=torch.int16, device="cuda")
    m = pkg.HIPMatcher(width=W6, height=H6, max_batch=n, **hip_kw(KW6))
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        m.compute_device(dL, dR, dD, s.cuda_stream)
    s.synchronize()
    assert m.search_variant.startswith("generic_dslice")
    m.close()
    got = dD.cpu().numpy()
    for i in range(n):
        assert_same(got[i], oracle.bm_compute(Ls[i], Rs[i], **KW6), "frame %d" % i)


def test_compute_batch_page_locked_and_pageable(pkg, oracle, synth):
    import torch
    n = 4
    Ls, Rs = synth.make_stream(7500, n, W6, H6, D6)
    pl, pr = torch.from_numpy(Ls).pin_memory(), torch.from_numpy(Rs).pin_memory()
    po = torch.full((n, H6, W6), 12345, dtype=torch.int16).pin_memory()
    m = pkg.HIPMatcher(width=W6, height=H6, max_batch=2, **hip_kw(KW6))
    got = m.compute_batch(pl.numpy(), pr.numpy(), po.numpy())
    again = m.compute_batch(Ls, Rs)
    m.close()
    assert np.array_equal(got, again)
    for i in range(n):
        assert_same(got[i], oracle.bm_compute(Ls[i], Rs[i], **KW6), "frame %d" % i)


def test_set_roi1_and_roi2(pkg, oracle, synth):
    L, R = synth.make_pair(synth.STREAM_SEED + 7600, W6, H6, D6)
    roi1, roi2 = (350, 10, 200, 50), (20, 5, 600, 60)
    got, want, variant = run(pkg, oracle, L, R, roi1=roi1, roi2=roi2, **KW6)
    assert variant.startswith("generic_dslice")
    assert_same(got, want)
    assert (want != -16).any()


def test_legacy_right_clamp(pkg, oracle, synth):
    L, R = synth.make_pair(synth.STREAM_SEED + 7700, W6, H6, D6)
    got, want, variant = run(pkg, oracle, L, R, legacy=1, **KW6)
    assert variant.startswith("generic_dslice")
    assert_same(got, want)


Q_TEST = np.array([[1, 0, 0, -320.3], [0, 1, 0, -36.8], [0, 0, 0, 700.25], [0, 0, 1 / 12.0, 0.0]])


def test_compute_depth(pkg, oracle, synth):
    L, R = synth.make_pair(synth.STREAM_SEED + 7800, W6, H6, D6)
    mask = ((L > 100) * 255).astype(np.uint8)
    regions = [(330, 8, 200, 50), (0, 0, W6, H6), (500, 30, 60, 20)]
    m = pkg.HIPMatcher(width=W6, height=H6, **hip_kw(KW6))
    mean, cnt, disp = m.compute_depth(L, R, Q_TEST, mask, regions, calibration_unit=25.0, want_disp=True)
    assert m.search_variant.startswith("generic_dslice")
    m.close()
    want_disp = oracle.bm_compute(L, R, **KW6)
    assert_same(disp, want_disp)
    wm, wc = oracle.depth_stats(want_disp, Q_TEST, mask, regions, 25.0)
    assert np.array_equal(cnt, wc) and wc[1] > 1000
    assert np.allclose(mean, wm, rtol=1e-9, atol=0)


# ---- 7. configurations that worked before keep their kernels -----------------------------------------------------------
# (expected strings recorded with the library of the parent tree on an MI355X)
UNCHANGED = [
    (dict(numDisparities=64, blockSize=9), 320, 100, 0, "fast_qsad"),
    (dict(numDisparities=192, blockSize=13), 1280, 720, -1, "fast_ring8_qsad"),
    (dict(numDisparities=64, blockSize=25, preFilterCap=31), 320, 100, -1, "generic_u16"),
    (dict(numDisparities=64, blockSize=25, preFilterCap=63), 320, 100, -1, "generic_u32"),
    (dict(numDisparities=256, blockSize=31, preFilterCap=15), 480, 80, -1, "generic_u16"),
]


@pytest.mark.parametrize("kw,W,H,mode,variant", UNCHANGED)
def test_selection_of_configurations_that_worked_before(pkg, oracle, synth, kw, W, H, mode, variant):
    L, R = synth.make_pair(synth.STREAM_SEED + 7900 + W, W, H, kw["numDisparities"])
    pkg.binding.lib().rtdm_debug_search_kernel(mode)
    try:
        got, want, got_variant = run(pkg, oracle, L, R, **kw)
    finally:
        pkg.binding.lib().rtdm_debug_search_kernel(-1)
    assert got_variant == variant
    assert_same(got, want)
