"""The disparity WLS post-filter without a GPU: the NumPy restatement (tests/wls_ref.py) against dense solves and hand-made
maps, the W1 / W2 helpers of the C ABI against their formulas, and rtdm_wls_create's parameter checks."""
import ctypes as C
import math

import numpy as np
import pytest

import wls_ref as ref
from conftest import load


def test_thomas_equals_a_dense_solve():
    rng = np.random.default_rng(0)
    for L in (1, 2, 7, 33):
        w = rng.random((3, L)).astype(np.float32).astype(np.float64)
        w[:, 0] = 0
        a, b, c = ref.pass_matrices(w, 1234.5)
        f = rng.normal(size=(3, L, 2)) * 100
        u = ref.thomas(a, b, c, f)
        for i in range(3):
            M = np.diag(b[i]) + np.diag(a[i, 1:], -1) + np.diag(c[i, :-1], 1)
            assert np.allclose(u[i], np.linalg.solve(M, f[i]), rtol=1e-9, atol=1e-9)


def test_fgs_equals_dense_passes():
    rng = np.random.default_rng(1)
    h, w = 5, 6
    G = rng.integers(0, 255, (h, w)).astype(np.uint8)
    p = dict(lambda_=50.0, sigma_color=20.0, num_iter=2, attenuation=0.25)
    wh, wv = ref.weights(G, ref.lut(p["sigma_color"]).astype(np.float64), (0, w, 0, h))
    f = rng.normal(size=(h, w, 1))
    u = ref.fgs(f, wh, wv, p)
    v = f[..., 0].copy()
    for lam in ref.lambdas(p):
        for rows in (True, False):
            x = v if rows else v.T
            ww = wh if rows else wv.T
            out = np.empty_like(x)
            for i in range(x.shape[0]):
                n = x.shape[1]
                M = np.eye(n)
                for j in range(1, n):
                    M[j, j - 1] -= lam * ww[i, j]; M[j - 1, j] -= lam * ww[i, j]
                    M[j, j] += lam * ww[i, j]; M[j - 1, j - 1] += lam * ww[i, j]
                out[i] = np.linalg.solve(M, x[i])
            v = out if rows else out.T
    assert np.allclose(u[..., 0], v, rtol=1e-9, atol=1e-9)


def base_params(r=1, T=24):
    return dict(lambda_=8000.0, sigma_color=1.5, lrc_thresh=T, depth_discontinuity_radius=r, min_disparity=0,
                num_disparities=16, roi_left=0, roi_right=0, roi_top=0, roi_bottom=0, num_iter=3, attenuation=0.25,
                use_confidence=1)


def test_confidence_on_hand_made_maps():
    W, H = 12, 9
    p = base_params(r=1)
    dL = np.full((H, W), 3 * 16, np.int16)
    dR = np.full((H, W), -3 * 16, np.int16)
    C0 = ref.confidence(dL, dR, p)
    assert (C0[:, 3:] == 255).all()
    assert (C0[:, :3] == 0).all()                  # x' = x - 3 < 0: outside the frame
    dL2 = dL.copy(); dL2[4, 6] = -16               # invalid left value
    assert ref.confidence(dL2, dR, p)[4, 6] == 0
    dR2 = dR.copy(); dR2[2, 5] = -16 * 16          # invalid right value at x' = 5 of (2, 8)
    assert ref.confidence(dL, dR2, p)[2, 8] == 0
    dR3 = dR.copy(); dR3[6, 4] = -3 * 16 - 25      # |dL + dR| = 25 > T
    assert ref.confidence(dL, dR3, p)[6, 7] == 0
    dR4 = dR.copy(); dR4[6, 4] = -3 * 16 - 24      # = T passes, and the discontinuity is not above T
    assert ref.confidence(dL, dR4, p)[6, 7] == 255
    # a depth step of more than T at distance r + 1 leaves the pixel alone, at distance r it clears it
    dL5 = dL.copy(); dL5[:, 9:] = 3 * 16 + 25
    C5 = ref.confidence(dL5, np.full((H, W), -3 * 16, np.int16), p)
    assert C5[4, 7] == 255 and C5[4, 8] == 0
    # a window with a single valid value is never a discontinuity
    dL6 = np.full((H, W), -16, np.int16); dL6[4, 6] = 3 * 16
    assert ref.confidence(dL6, dR, p)[4, 6] == 255


def test_lambda_zero_and_constant_and_bounds():
    rng = np.random.default_rng(2)
    W, H = 30, 20
    G = rng.integers(0, 255, (H, W)).astype(np.uint8)
    dL = (rng.integers(2, 12, (H, W)) * 16).astype(np.int16)
    dR = np.full((H, W), -16 * 16, np.int16)
    for y in range(H):
        for x in range(W):
            xp = x - dL[y, x] // 16
            if xp >= 0:
                dR[y, xp] = -dL[y, x]
    p = base_params(r=0)
    p["lambda_"] = 0.0
    res = ref.wls_filter(dL, G, p, dR)
    C = res["conf"]
    assert (C > 0).any()
    assert np.array_equal(res["out"][C > 0], dL[C > 0]) and (res["out"][C == 0] == -16).all()
    p["lambda_"] = 8000.0
    res = ref.wls_filter(dL, G, p, dR)
    v = res["filtered"][res["out"] != -16]
    assert v.min() >= dL[C > 0].min() - 1e-9 and v.max() <= dL[C > 0].max() + 1e-9
    cst = np.full((H, W), 5 * 16, np.int16)
    res = ref.wls_filter(cst, G, p, np.full((H, W), -5 * 16, np.int16))
    assert (res["out"][:, 5:] == 80).all() and np.allclose(res["filtered"][:, 5:], 80.0, rtol=1e-12)


def test_lut_is_float_and_flushed():
    t = ref.lut(1.5)
    assert t.dtype == np.float32 and t[0] == 1.0 and t[-1] == 0.0
    assert (t[t > 0] >= np.finfo(np.float32).tiny).all()
    assert t[100] == np.float32(math.exp(-10 / 1.5))


def test_abi_helpers_match_the_formulas():
    B = load("binding")
    L = B.lib()
    for blk, minD, D in ((9, 0, 64), (13, -16, 48), (21, -100, 32)):
        bp = B.make_params(blockSize=blk, minDisparity=minD, numDisparities=D, preFilterCap=17)
        w = B.WLSParams()
        assert L.rtdm_wls_params_for_bm(C.byref(bp), C.byref(w)) == 0
        want = ref.params_for_bm(blk, minD, D)
        for k, v in want.items():
            assert getattr(w, k) == v, (k, getattr(w, k), v)
        r = B.BMParams()
        assert L.rtdm_bm_right_params(C.byref(bp), C.byref(r)) == 0
        assert (r.minDisparity, r.numDisparities, r.blockSize, r.preFilterCap, r.textureThreshold, r.uniquenessRatio,
                r.speckleWindowSize, r.disp12MaxDiff) == (-(minD + D) + 1, D, blk, 17, 0, 0, 0, 1000000)
        sp = B.SGMParams(blk, minD, D, 600, 2400, 10, 100, 32, 1, 5)
        assert L.rtdm_wls_params_for_sgm(C.byref(sp), C.byref(w)) == 0
        for k, v in ref.params_for_sgm(blk, minD, D).items():
            assert getattr(w, k) == v, (k, getattr(w, k), v)
        rs = B.SGMParams()
        assert L.rtdm_sgm_right_params(C.byref(sp), C.byref(rs)) == 0
        assert (rs.minDisparity, rs.numDisparities, rs.blockSize, rs.P1, rs.P2, rs.paths, rs.uniquenessRatio,
                rs.speckleWindowSize, rs.disp12MaxDiff) == (-(minD + D) + 1, D, blk, 600, 2400, 5, 0, 0, 1000000)
    assert L.rtdm_wls_params_for_bm(None, C.byref(w)) == -7


def test_create_refuses_bad_parameters_before_the_device():
    import torch
    B = load("binding")
    L = B.lib()
    h = C.c_void_p()

    def params(**kw):
        p = B.WLSParams()
        for k, v in dict(base_params(), **kw).items():
            setattr(p, k, v)
        return p
    for bad in (dict(lambda_=-1.0), dict(sigma_color=0.0), dict(lrc_thresh=-1), dict(depth_discontinuity_radius=-1),
                dict(roi_left=-1), dict(roi_bottom=-2), dict(num_iter=0), dict(num_iter=17), dict(attenuation=0.0),
                dict(attenuation=1.5), dict(use_confidence=2)):
        assert L.rtdm_wls_create(C.byref(params(**bad)), 64, 48, 1, 0, C.byref(h)) == -1, bad
    assert L.rtdm_wls_create(None, 64, 48, 1, 0, C.byref(h)) == -7
    assert L.rtdm_wls_create(C.byref(params()), 4097, 48, 1, 0, C.byref(h)) == -6
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    assert L.rtdm_wls_create(C.byref(params()), 64, 48, 1, 0, C.byref(h)) == -3
