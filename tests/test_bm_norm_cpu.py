"""No-GPU checks of StereoBM's preFilterType NORMALIZED_RESPONSE / preFilterSize: the two formulations of the prefilter in
tests/bm_norm_ref.py agree with each other, the chain bm_norm_ref builds around the oracle's stages reproduces
oracle.bm_compute when it is handed the oracle's own x-Sobel, the inputs of the GPU tests are useful ones, and the new
symbols, constants and keywords exist.  (That the formulations agree with each other says nothing about the library: parity
is unpinned.)"""
import ctypes as C
import inspect

import numpy as np
import pytest

import bm_norm_ref as ref
from conftest import load

SIZES = [5, 7, 9, 11, 21, 49, 63, 91, 255]
CAPS = [1, 31, 63]


def _images(H, W, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    single = np.zeros((H, W), np.uint8); single[H // 2, W // 3] = 255
    return {"random": rng.integers(0, 256, (H, W)).astype(np.uint8),
            "smooth": (127 + 100 * np.sin(xx / 7.0) * np.cos(yy / 5.0)).astype(np.uint8),
            "zeros": np.zeros((H, W), np.uint8), "full": np.full((H, W), 255, np.uint8), "single": single,
            "checker": (((xx + yy) & 1) * 255).astype(np.uint8), "blocks": ((((xx // 8) + (yy // 8)) & 1) * 255).astype(np.uint8)}


@pytest.mark.parametrize("ws", SIZES)
def test_closed_form_equals_the_loop(ws):
    r = ws // 2
    shapes = [(max(r, 2) + 9, 70), (max(r, 2), 6), (max(r, 2) + 1, 33), (140, 6)]
    for H, W in shapes:
        for name, img in _images(H, W, 17 * ws + H).items():
            for cap in CAPS:
                a = ref.prefilter_norm(img, ws, cap)
                try:
                    b = ref.prefilter_norm_loop(img, ws, cap)
                except ref.TableIndexError:
                    assert not ref.table_safe(ws), (ws, name)       # only the sizes DESIGN.md lists may leave the table
                    continue
                assert np.array_equal(a, b), (ws, cap, H, W, name)


def test_table_hazard_sizes_are_the_documented_ones():
    unsafe = [ws for ws in range(5, 256, 2) if not ref.table_safe(ws)]
    assert unsafe == [51, 73, 75, 77, 79, 81, 83, 85, 87, 89]
    assert ref.max_abs_val(89) == (1971, -1972) and ref.max_abs_val(51)[1] == -1293


@pytest.mark.parametrize("ws", [5, 9, 21, 63, 91, 255])
def test_frames_lower_than_the_window_radius(ws):
    r = ws // 2
    for H in (1, 2, max(r - 1, 1)):
        img = np.random.default_rng(ws + H).integers(0, 256, (H, 40)).astype(np.uint8)
        got = ref.prefilter_norm(img, ws, 31)
        # brute force N2-N5 at a few pixels
        sc_s, sc_g = ref.scales(ws)
        a = img.astype(int)
        for (y, x) in [(0, 0), (H - 1, 39), (H // 2, 17)]:
            S = sum(a[min(max(y + dy, 0), H - 1), min(max(x + dx, 0), 39)] for dy in range(-r, r + 1) for dx in range(-r, r + 1))
            cl = lambda yy, xx: a[min(max(yy, 0), H - 1), min(max(xx, 0), 39)]
            n = 4 * cl(y, x) + cl(y, x - 1) + cl(y, x + 1) + cl(y - 1, x) + cl(y + 1, x)
            assert got[y, x] == min(max((n * sc_g - S * sc_s) >> 10, -31), 31) + 31


@pytest.mark.parametrize("ws", [91, 93, 127, 255])
@pytest.mark.parametrize("cap", CAPS)
def test_large_windows_give_the_constant_cap(ws, cap):
    assert ref.scales(ws) == (0, 0)
    img = np.random.default_rng(ws).integers(0, 256, (37, 53)).astype(np.uint8)
    assert (ref.prefilter_norm(img, ws, cap) == cap).all()
    assert (ref.prefilter_norm_loop(np.tile(img, (8, 1)), ws, cap) == cap).all()


@pytest.mark.parametrize("kw,W,H,rois,legacy", [
    (dict(numDisparities=32, blockSize=9), 160, 120, (None, None), False),
    (dict(numDisparities=64, blockSize=13, minDisparity=-7, preFilterCap=15, uniquenessRatio=0, speckleWindowSize=20,
          speckleRange=4, disp12MaxDiff=0), 233, 77, ((40, 10, 150, 60), (5, 3, 220, 70)), False),
    (dict(numDisparities=48, blockSize=7, minDisparity=3, textureThreshold=0, disp12MaxDiff=1), 200, 64, (None, None), True),
])
def test_the_chain_with_xsobel_is_the_oracle(oracle, synth, kw, W, H, rois, legacy):
    L, R = synth.make_pair(synth.STREAM_SEED + 8100 + W, W, H, kw["numDisparities"])
    got = ref.bm_chain(L, R, oracle.prefilter_xsobel, legacy=legacy, roi1=rois[0], roi2=rois[1], **kw)
    oracle.set_legacy_right_clamp(legacy)
    try:
        want = oracle.bm_compute(L, R, roi1=rois[0], roi2=rois[1], **kw)
    finally:
        oracle.set_legacy_right_clamp(False)
    assert np.array_equal(got, want)
    assert (want != (kw.get("minDisparity", 0) - 1) * 16).any()


# the pairs of tests/test_gpu_bm_norm.py::test_reference_literals: a condition on the INPUT, checked on the reference alone
LITERAL_CASES = [(D, ws) for D in (64, 192) for ws in (5, 9, 21)]


def literal_pair(synth, D):
    W, H = (480, 160) if D == 64 else (640, 120)
    return synth.make_pair(synth.STREAM_SEED + 8200 + D, W, H, D)


@pytest.mark.parametrize("D,ws", LITERAL_CASES)
def test_reference_literal_pairs_are_useful(oracle, synth, D, ws):
    L, R = literal_pair(synth, D)
    kw = dict(numDisparities=D, blockSize=13, preFilterCap=31)
    want = ref.bm_compute_norm(L, R, ws, **kw)
    assert (want != -16).mean() > 0.05
    assert not np.array_equal(want, oracle.bm_compute(L, R, **kw))


def test_symbols_exist_and_null_handles_are_refused():
    B = load("binding")
    L = B.lib()
    assert "rtdm_bm_set_prefilter" in B.EXPORTS and "rtdm_bm_get_prefilter" in B.EXPORTS
    assert L.rtdm_bm_set_prefilter(None, 1, 9) == -7
    t, s = C.c_int(-5), C.c_int(-5)
    assert L.rtdm_bm_get_prefilter(None, C.byref(t), C.byref(s)) == -7
    assert L.rtdm_abi_version() == 3


def test_python_constants_and_keywords():
    pkg = load()
    assert (pkg.PREFILTER_NORMALIZED_RESPONSE, pkg.PREFILTER_XSOBEL) == (0, 1)      # cv::StereoBM's values
    sig = inspect.signature(pkg.HIPMatcher.__init__)
    assert sig.parameters["preFilterType"].default == pkg.PREFILTER_XSOBEL
    assert sig.parameters["preFilterSize"].default == 9
    for name in ("setPreFilterType", "setPreFilterSize", "getPreFilterType", "getPreFilterSize"):
        assert callable(getattr(pkg.HIPMatcher, name))


def test_header_declares_the_constants():
    import os
    import re
    from conftest import ROOT
    text = open(os.path.join(ROOT, "include", "rtdm.h")).read()
    assert re.search(r"#define RTDM_PREFILTER_NORMALIZED_RESPONSE 0\b", text)
    assert re.search(r"#define RTDM_PREFILTER_XSOBEL 1\b", text)
