"""The disparity WLS post-filter on the device (rtdm_wls_*, rtdm_bm_compute_filtered): the right matchers against the oracle,
the confidence bit for bit and the filtered maps within tolerance against tests/wls_ref.py, the filter's properties, batching,
repeatability and the error paths."""
import ctypes as C

import numpy as np
import pytest

import wls_ref as ref
from conftest import load

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    import torch                         # torch first: it brings its own HIP runtime and must initialise before ours
    assert torch.cuda.is_available(), "the -m gpu suite needs an MI355X"
    return load()


def wparams(pkg, p):
    w = pkg.binding.WLSParams()
    for k, v in p.items():
        setattr(w, k, v)
    return w


def check_against_ref(got, fl, conf, want, box_only=True):
    """confidence bit for bit; float within 1e-4 relative where F2_ref >= 1; int16 within 1 LSB there and equal on >= 99.9 %
    of the ROI"""
    bad = np.argwhere(conf != want["conf"])
    assert len(bad) == 0, "confidence differs on %d pixels; first at %s: %g, want %g" % (
        len(bad), tuple(bad[0]), conf[tuple(bad[0])], want["conf"][tuple(bad[0])])
    F2 = want["F2"]
    strong = np.nan_to_num(F2, nan=0.0) >= 1.0
    if strong.any():
        wf = want["filtered"][strong]
        rel = np.abs(fl[strong].astype(np.float64) - wf) / np.maximum(np.abs(wf), 1.0)
        i = int(np.argmax(rel))
        assert rel.max() <= 1e-4, "float output off by %.3g relative at %s: %r, want %r (F2 %r)" % (
            rel.max(), tuple(np.argwhere(strong)[i]), fl[strong][i], wf[i], F2[strong][i])
        assert np.abs(got[strong].astype(np.int32) - want["out"][strong]).max() <= 1
    outside = np.isnan(F2)
    assert np.array_equal(got[outside], want["out"][outside])
    # Where F2 nears the bottom of the float range (below FLT_MIN it is gone: fp32 solves, as in the library) F1 / F2 loses its
    # digits; the equality count runs over the ROI pixels whose F2_ref is a normal float with 2^26 to spare (DESIGN.md W7 hazard)
    roi = np.nan_to_num(F2, nan=0.0) >= 1e-30
    if roi.any():
        eq = (got[roi] == want["out"][roi]).mean()
        bad = np.argwhere(roi & (got != want["out"]))
        assert eq >= 0.999, "int16 output equal on %.5f of the ROI; first at %s: %d, want %d (F2 %r)" % (
            eq, tuple(bad[0]), got[tuple(bad[0])], want["out"][tuple(bad[0])], F2[tuple(bad[0])])


def matcher_pair(pkg, kind, W, H, D, w, minD=0, paths=5):
    if kind == "bm":
        m = pkg.HIPMatcher(numOfDisparities=D, blockSize=w, minDisparity=minD, width=W, height=H)
    else:
        m = pkg.HIPSemiGlobalMatcher(blockSize=w, minDisparity=minD, numOfDisparities=D, width=W, height=H, paths=paths)
    return m, pkg.create_right_matcher(m)


def frames(pkg, W, H, D, seed=0, cn=1):
    s = pkg.synth
    L, R = s.make_pair(s.STREAM_SEED + 300 + seed, W, H, D)
    if cn == 3:
        Lc, _ = s.make_pair(s.STREAM_SEED + 900 + seed, W, H, D)
        G = np.stack([L, Lc, (L.astype(np.int32) * 3 // 4).astype(np.uint8)], axis=2)
    else:
        G = L
    return L, R, np.ascontiguousarray(G)


# ---- W1: the right matchers ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,D,w,minD,paths", [("bm", 64, 9, 0, 5), ("bm", 32, 13, -16, 5), ("sgm", 64, 5, 0, 5),
                                                 ("sgm", 48, 7, -8, 8)])
def test_right_matcher_equals_the_oracle_on_swapped_images(pkg, oracle, kind, D, w, minD, paths):
    W, H = 192, 96
    L, R, _ = frames(pkg, W, H, D)
    m, rm = matcher_pair(pkg, kind, W, H, D, w, minD, paths)
    got = rm.compute(R, L)
    minDR = -(minD + D) + 1
    if kind == "bm":
        want = oracle.bm_compute(R, L, numDisparities=D, blockSize=w, minDisparity=minDR, textureThreshold=0,
                                 uniquenessRatio=0, speckleWindowSize=0, disp12MaxDiff=1000000)
    else:
        want = oracle.sgm_compute(R, L, blockSize=w, minDisparity=minDR, numDisparities=D, uniquenessRatio=0,
                                  speckleWindowSize=0, disp12MaxDiff=1000000, paths=paths)
    assert np.array_equal(got, want), "%d pixels differ" % int((got != want).sum())


# ---- the filter against the reference -----------------------------------------------------------------------------------
CONFIGS = [
    # kind, W, H, D, blockSize, minD, paths, channels
    ("bm", 160, 120, 64, 9, 0, 5, 1),
    ("bm", 200, 100, 32, 5, 0, 5, 3),
    ("bm", 180, 90, 16, 21, -16, 5, 1),
    ("bm", 1280, 720, 64, 9, 0, 5, 1),
    ("sgm", 160, 96, 64, 5, 0, 5, 1),
    ("sgm", 150, 80, 32, 7, -8, 8, 3),
    ("sgm", 63, 40, 16, 3, 0, 8, 1),
    ("bm", 65, 48, 16, 5, 0, 5, 1),
]


@pytest.mark.parametrize("kind,W,H,D,w,minD,paths,cn", CONFIGS)
def test_filter_matches_the_reference(pkg, kind, W, H, D, w, minD, paths, cn):
    L, R, G = frames(pkg, W, H, D, seed=W + H, cn=cn)
    m, rm = matcher_pair(pkg, kind, W, H, D, w, minD, paths)
    dL, dR = m.compute(L, R), rm.compute(R, L)
    f = pkg.create_disparity_wls_filter(m)
    got, fl = f.filter(dL, G, None, dR, want_float=True)
    p = (ref.params_for_bm if kind == "bm" else ref.params_for_sgm)(m.params.blockSize, minD, D)
    want = ref.wls_filter(dL, G, p, dR)
    check_against_ref(got, fl, f.getConfidenceMap(), want)
    assert (want["conf"] > 0).any()


def synthetic_maps(W, H, minD=0, D=32, seed=1):
    """dL with steps and holes, dR consistent with it on most pixels, a textured guide"""
    rng = np.random.default_rng(seed)
    x = np.arange(W)[None, :]
    y = np.arange(H)[:, None]
    d = (4 + (x * 7 // max(W, 1)) + 6 * ((x // 17 + y // 11) % 2)) * 16 + (x + y) % 5
    d = np.clip(d, minD * 16, (minD + D - 1) * 16)
    dL = d.astype(np.int16)
    dL[rng.random((H, W)) < 0.1] = (minD - 1) * 16
    invR = -(minD + D) * 16
    dR = np.full((H, W), invR, np.int16)
    for yy in range(H):
        for xx in range(W):
            if dL[yy, xx] != (minD - 1) * 16:
                xp = xx - int(dL[yy, xx] / 16)
                if 0 <= xp < W:
                    dR[yy, xp] = -dL[yy, xx] + int(rng.integers(-3, 4) if rng.random() > 0.01 else rng.integers(-40, 41))
    G = (rng.integers(0, 40, (H, W)) + 100 * ((x // 23) % 2)).astype(np.uint8)
    return dL, dR, G


def generic_params(minD=0, D=32, r=2, off=(0, 0, 0, 0), use_confidence=1):
    p = dict(lambda_=8000.0, sigma_color=1.5, lrc_thresh=24, depth_discontinuity_radius=r, min_disparity=minD,
             num_disparities=D, roi_left=off[0], roi_right=off[1], roi_top=off[2], roi_bottom=off[3], num_iter=3,
             attenuation=0.25, use_confidence=use_confidence)
    return p


@pytest.mark.parametrize("W,H", [(1, 40), (63, 1), (65, 2), (4096, 6), (97, 720)])
def test_frame_shapes(pkg, W, H):
    dL, dR, G = synthetic_maps(W, H)
    p = generic_params(off=(0, 0, 0, 0))
    f = pkg.HIPDisparityWLSFilter(wparams(pkg, p), W, H)
    got, fl = f.filter(dL, G, None, dR, want_float=True)
    check_against_ref(got, fl, f.getConfidenceMap(), ref.wls_filter(dL, G, p, dR))


def test_negative_min_disparity_and_radius_128(pkg):
    W, H = 300, 40
    dL, dR, G = synthetic_maps(W, H, minD=-10, D=48)
    x = np.arange(W)[None, :].repeat(H, 0)
    dL = np.where(dL == -11 * 16, dL, 5 * 16 + x % 7 + 40 * (x >= 280)).astype(np.int16)   # one step, 128+ columns away
    dR = np.full((H, W), -38 * 16, np.int16)
    for yy in range(H):
        for xx in range(W):
            if dL[yy, xx] != -11 * 16 and xx - int(dL[yy, xx] / 16) >= 0:
                dR[yy, xx - int(dL[yy, xx] / 16)] = -dL[yy, xx]
    p = generic_params(minD=-10, D=48, r=128, off=(3, 2, 1, 4))
    assert (ref.confidence(dL, dR, p) > 0).mean() > 0.2
    f = pkg.HIPDisparityWLSFilter(wparams(pkg, p), W, H)
    got, fl = f.filter(dL, G, None, dR, want_float=True)
    check_against_ref(got, fl, f.getConfidenceMap(), ref.wls_filter(dL, G, p, dR))


def test_empty_roi_is_all_invalid(pkg):
    W, H, D = 64, 48, 64
    L, R, G = frames(pkg, W, H, D)
    m, rm = matcher_pair(pkg, "bm", W, H, D, 9)
    f = pkg.create_disparity_wls_filter(m)
    assert f.getROI() == (0, 0, 0, 0)
    got = f.filter(m.compute(L, R), G, None, rm.compute(R, L))
    assert (got == -16).all() and (f.getConfidenceMap() == 0).all()


def test_without_confidence(pkg):
    dL, _, G = synthetic_maps(120, 50)
    p = generic_params(off=(5, 0, 2, 3), use_confidence=0)
    f = pkg.HIPDisparityWLSFilter(wparams(pkg, p), 120, 50)
    got, fl = f.filter(dL, G, None, None, want_float=True)
    want = ref.wls_filter(dL, G, p)
    roi = ~np.isnan(want["F1"])
    # without the confidence the ratio does not cancel the solve's rounding: (I + lambda L) has a condition number up to ~1e4
    rel = np.abs(fl[roi] - want["filtered"][roi]) / np.maximum(np.abs(want["filtered"][roi]), 1.0)
    assert rel.max() <= 2e-3
    assert np.abs(got.astype(np.int32) - want["out"]).max() <= 1 and (got == want["out"]).mean() >= 0.99
    assert (f.getConfidenceMap() == 0).all()


# ---- properties --------------------------------------------------------------------------------------------------------
def test_lambda_zero_returns_the_confident_input(pkg):
    dL, dR, G = synthetic_maps(80, 40)
    p = generic_params()
    f = pkg.HIPDisparityWLSFilter(wparams(pkg, p), 80, 40)
    f.setLambda(0)
    got = f.filter(dL, G, None, dR)
    C = f.getConfidenceMap()
    assert (C > 0).any()
    assert np.array_equal(got[C > 0], dL[C > 0]) and (got[C == 0] == -16).all()


def test_constant_map_stays_constant_and_output_is_bounded(pkg):
    W, H = 100, 60
    _, _, G = synthetic_maps(W, H)
    dL = np.full((H, W), 20 * 16, np.int16)
    dR = np.full((H, W), -20 * 16, np.int16)
    p = generic_params(off=(20, 0, 0, 0))
    f = pkg.HIPDisparityWLSFilter(wparams(pkg, p), W, H)
    got = f.filter(dL, G, None, dR)
    assert (got[:, 20:] == 320).all() and (got[:, :20] == -16).all()
    dL, dR, G = synthetic_maps(W, H, seed=5)
    got, fl = f.filter(dL, G, None, dR, want_float=True)
    C = f.getConfidenceMap()
    lo, hi = dL[C > 0].min(), dL[C > 0].max()
    v = fl[got != -16]
    assert v.min() >= lo - 1e-2 and v.max() <= hi + 1e-2


def test_edge_aware(pkg):
    W, H = 120, 30
    dL = np.where(np.arange(W)[None, :] < 60, 10 * 16, 30 * 16).repeat(H, 0).astype(np.int16)
    p = generic_params(use_confidence=0)
    f = pkg.HIPDisparityWLSFilter(wparams(pkg, p), W, H)
    edge = np.where(np.arange(W)[None, :] < 60, 20, 220).repeat(H, 0).astype(np.uint8)
    flat = np.full((H, W), 128, np.uint8)
    sharp = f.filter(dL, edge)
    soft = f.filter(dL, flat)
    assert abs(int(sharp[15, 59]) - 160) <= 2 and abs(int(sharp[15, 60]) - 480) <= 2
    assert abs(int(soft[15, 59]) - 160) > 60 and abs(int(soft[15, 60]) - 480) > 60


# ---- batching, repeatability, the one-call form ----------------------------------------------------------------------------
def test_batches_and_repeatability(pkg):
    import torch
    W, H, mb = 96, 64, 2
    n = 2 * mb + 1
    p = generic_params(off=(4, 1, 2, 0))
    f = pkg.HIPDisparityWLSFilter(wparams(pkg, p), W, H, max_batch=mb)
    maps = [synthetic_maps(W, H, seed=10 + i) for i in range(n)]
    dl = torch.tensor(np.stack([m[0] for m in maps])).cuda()
    dr = torch.tensor(np.stack([m[1] for m in maps])).cuda()
    dg = torch.tensor(np.stack([m[2] for m in maps])).cuda()
    out = torch.empty((n, H, W), dtype=torch.int16, device="cuda")
    conf = torch.empty((n, H, W), dtype=torch.float32, device="cuda")
    flt = torch.empty((n, H, W), dtype=torch.float32, device="cuda")
    f.filter_device(dl, dr, dg, out, conf, flt)
    torch.cuda.synchronize()
    for i in range(n):
        one_out = torch.empty((1, H, W), dtype=torch.int16, device="cuda")
        f.filter_device(dl[i:i + 1], dr[i:i + 1], dg[i:i + 1], one_out)
        torch.cuda.synchronize()
        assert torch.equal(one_out[0], out[i])
        host, hf = f.filter(maps[i][0], maps[i][2], None, maps[i][1], want_float=True)
        assert np.array_equal(host, out[i].cpu().numpy())
        assert np.array_equal(hf.view(np.int32), flt[i].cpu().numpy().view(np.int32))
        assert np.array_equal(f.getConfidenceMap(), conf[i].cpu().numpy())
        again, af = f.filter(maps[i][0], maps[i][2], None, maps[i][1], want_float=True)
        assert np.array_equal(again, host) and np.array_equal(af.view(np.int32), hf.view(np.int32))


def test_compute_filtered_equals_the_three_steps(pkg):
    W, H, D, w = 320, 180, 64, 9
    L, R, _ = frames(pkg, W, H, D, seed=3)
    m, rm = matcher_pair(pkg, "bm", W, H, D, w)
    f = pkg.create_disparity_wls_filter(m)
    got, raw = f.compute_filtered(m, rm, L, R, want_raw=True)
    dL = m.compute(L, R)
    assert np.array_equal(raw, dL)
    assert np.array_equal(got, f.filter(dL, L, None, rm.compute(R, L)))


def test_error_codes(pkg):
    B = pkg.binding
    lib = B.lib()
    W, H = 64, 32
    p = generic_params()
    f = pkg.HIPDisparityWLSFilter(wparams(pkg, p), W, H)
    d = np.zeros((H, W), np.int16)
    g = np.zeros((H, W, 3), np.uint8)
    o = np.zeros((H, W), np.int16)
    call = lambda cn, w, h, dl=d.ctypes.data, dr=d.ctypes.data, gg=g.ctypes.data, oo=o.ctypes.data: lib.rtdm_wls_filter(
        f._h, dl, W * 2, dr, W * 2, gg, W * 3, cn, w, h, oo, W * 2, None, 0, None, 0)
    assert call(1, W, H) == 0 and call(3, W, H) == 0
    assert call(2, W, H) == -1
    assert call(1, W + 1, H) == -2 and call(1, W, H + 1) == -2
    assert call(1, W, H, dl=None) == -7 and call(1, W, H, dr=None) == -7
    assert call(1, W, H, gg=None) == -7 and call(1, W, H, oo=None) == -7
    h = C.c_void_p()
    assert lib.rtdm_wls_create(C.byref(wparams(pkg, p)), 4097, 16, 1, 0, C.byref(h)) == -6
    assert lib.rtdm_wls_create(C.byref(wparams(pkg, p)), 16, 4097, 1, 0, C.byref(h)) == -6
    with pytest.raises(ValueError):
        f.filter(d, g[:, :, 0], None, None)
