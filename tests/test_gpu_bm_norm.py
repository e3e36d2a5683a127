"""StereoBM with preFilterType NORMALIZED_RESPONSE and preFilterSize on the device (k_prefilter_norm.hip, rtdm_bm_set_prefilter).
Every result is compared bit for bit with tests/bm_norm_ref.py: the normalised-response prefilter restated in NumPy (rules
N1-N5), chained through the oracle's own later stages."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import bm_norm_ref as ref
import rectify_util as ru
from conftest import ROOT, load
from test_bm_norm_cpu import LITERAL_CASES, literal_pair

pytestmark = pytest.mark.gpu

NORM, XSOBEL = ref.PREFILTER_NORMALIZED_RESPONSE, ref.PREFILTER_XSOBEL


@pytest.fixture(scope="module")
def pkg():
    import torch                         # torch first: it brings its own HIP runtime and must initialise before ours
    assert torch.cuda.is_available(), "the -m gpu suite needs an MI355X"
    return load()


def assert_same(got, want, what=""):
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError("%s: %d / %d pixels differ; first at (y,x)=%s got %d want %d" % (
            what, len(bad), got.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])]))


def hip_kw(kw):
    kw = dict(kw)
    kw["numOfDisparities"] = kw.pop("numDisparities")
    return kw


def run(pkg, L, R, ws, roi1=None, roi2=None, legacy=0, **kw):
    """-> (device result, reference result, variant string) with the normalised-response prefilter of size ws"""
    H, W = L.shape
    m = pkg.HIPMatcher(width=W, height=H, legacy_right_clamp=legacy, preFilterType=NORM, preFilterSize=ws, **hip_kw(kw))
    assert (m.getPreFilterType(), m.getPreFilterSize()) == (NORM, ws)
    if roi1: m.setROI1(roi1)
    if roi2: m.setROI2(roi2)
    got = m.compute(L, R)
    variant = m.search_variant
    m.close()
    want = ref.bm_compute_norm(L, R, ws, legacy=bool(legacy), roi1=roi1, roi2=roi2, **kw)
    return got, want, variant


def xsobel_variant(pkg, L, R, **kw):
    H, W = L.shape
    m = pkg.HIPMatcher(width=W, height=H, **hip_kw(kw))
    got = m.compute(L, R)
    v = m.search_variant
    m.close()
    return got, v


# ---- 1. the reference's literals ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,ws", LITERAL_CASES)
def test_reference_literals(pkg, oracle, synth, D, ws):
    L, R = literal_pair(synth, D)
    kw = dict(numDisparities=D, blockSize=13, preFilterCap=31)
    got, want, _ = run(pkg, L, R, ws, **kw)
    assert (want != -16).mean() > 0.05
    assert_same(got, want, "D=%d ws=%d" % (D, ws))
    xs, _ = xsobel_variant(pkg, L, R, **kw)
    assert_same(xs, oracle.bm_compute(L, R, nthreads=8, **kw), "xsobel")
    assert not np.array_equal(got, xs)                                  # the switch really switches


# ---- 2. every search family reads the new planes, and selection does not depend on the prefilter --------------------------
FAMILIES = [
    (dict(numDisparities=192, blockSize=13), 1280, 720, -1, "fast_ring"),
    (dict(numDisparities=64, blockSize=9), 320, 100, 0, "fast_qsad"),
    (dict(numDisparities=64, blockSize=25, preFilterCap=31), 320, 100, -1, "generic_u16"),
    (dict(numDisparities=64, blockSize=25, preFilterCap=63), 320, 100, -1, "generic_u32"),
    (dict(numDisparities=320, blockSize=13), 640, 72, -1, "generic_dslice_"),
]


@pytest.mark.parametrize("kw,W,H,mode,family", FAMILIES)
def test_every_search_family(pkg, synth, kw, W, H, mode, family):
    L, R = synth.make_pair(synth.STREAM_SEED + 8300 + W + kw["blockSize"], W, H, kw["numDisparities"])
    pkg.binding.lib().rtdm_debug_search_kernel(mode)
    try:
        got, want, variant = run(pkg, L, R, 9, **kw)
        _, xvariant = xsobel_variant(pkg, L, R, **kw)
    finally:
        pkg.binding.lib().rtdm_debug_search_kernel(-1)
    assert variant == xvariant and variant.startswith(family), (variant, xvariant)
    assert_same(got, want, variant)
    assert (want != -16).any()


# ---- 3. alignment classes and pitched views ------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", [(320, 61), (328, 50), (333, 47), (64, 33)])
@pytest.mark.parametrize("ws", [9, 21])
def test_device_tensors_of_every_alignment_class(pkg, synth, W, H, ws):
    # contiguous device tensors: W % 16 == 0 takes the 128-bit loader, everything else (W % 8 == 0 included) the byte-wise one
    import torch
    n, D, w = 3, 32, 7
    L, R = synth.make_stream(8400 + W, n, W, H, D)
    dL, dR = torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()
    guard = torch.full((n + 2, H, W), 12345, dtype=torch.int16, device="cuda")
    m = pkg.HIPMatcher(numOfDisparities=D, blockSize=w, width=W, height=H, max_batch=n, preFilterType=NORM, preFilterSize=ws)
    m.compute_device(dL, dR, guard[1:1 + n], torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = guard.cpu().numpy()
    m.close()
    assert (got[0] == 12345).all() and (got[-1] == 12345).all()
    for i in range(n):
        assert_same(got[1 + i], ref.bm_compute_norm(L[i], R[i], ws, numDisparities=D, blockSize=w), "W=%d frame %d" % (W, i))


@pytest.mark.parametrize("ox,ws", [(7, 9), (16, 5), (8, 63)])
def test_compute_with_pitched_views(pkg, synth, ox, ws):
    W, H, D = 350, 90, 48
    L, R = synth.make_pair(synth.STREAM_SEED + 8500 + ox, W, H, D)
    pad = np.full((H + 5, W + 51), 200, np.uint8)
    pl, pr = pad.copy(), pad.copy()
    pl[3:3 + H, ox:ox + W] = L; pr[3:3 + H, ox:ox + W] = R
    m = pkg.HIPMatcher(width=W, height=H, numOfDisparities=D, blockSize=11, preFilterType=NORM, preFilterSize=ws)
    outp = np.full((H + 2, W + 9), 999, np.int16)
    out = outp[1:1 + H, 3:3 + W]
    m.compute(pl[3:3 + H, ox:ox + W], pr[3:3 + H, ox:ox + W], out)
    m.close()
    assert_same(np.ascontiguousarray(out), ref.bm_compute_norm(L, R, ws, numDisparities=D, blockSize=11))
    assert (outp[0] == 999).all() and (outp[-1] == 999).all() and (outp[:, :3] == 999).all() and (outp[:, 3 + W:] == 999).all()


# ---- 4. extreme shapes ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H,D,w,ws", [
    (4096, 41, 64, 9, 9),          # the widest frame the matcher takes, odd height
    (4095, 23, 32, 7, 21),
    (200, 20, 32, 9, 63),          # H < ws / 2
    (120, 9, 16, 5, 41),
    (300, 40, 32, 9, 255),         # ws >= 91: the constant plane
    (300, 40, 32, 9, 91),
    (320, 120, 64, 9, 89),         # the largest window that is not constant
    (129, 33, 16, 5, 5), (128, 32, 16, 5, 7), (127, 31, 16, 5, 11),      # one tile, give or take a pixel
])
def test_extreme_shapes(pkg, synth, W, H, D, w, ws):
    L, R = synth.make_pair(synth.STREAM_SEED + 8600 + W + ws, W, H, D)
    kw = dict(numDisparities=D, blockSize=w, textureThreshold=0 if ws >= 91 else 10)
    got, want, _ = run(pkg, L, R, ws, **kw)
    assert_same(got, want, "%dx%d ws=%d" % (W, H, ws))
    if ws == 89:
        assert (want != -16).mean() > 0.05


@pytest.mark.parametrize("cap", [1, 63])
def test_adversarial_images_at_the_table_hazard_sizes(pkg, cap):
    # checkerboards and isolated pixels drive val to its extremes; N5's clamp is the definition where the library leaves its table
    W, H, D = 260, 100, 32
    yy, xx = np.mgrid[0:H, 0:W]
    rng = np.random.default_rng(cap)
    dots = (rng.random((H, W)) < 0.01).astype(np.uint8) * 255
    for ws in (51, 79, 89):
        for L in (dots, 255 - dots, (((xx // 3 + yy // 3) & 1) * 255).astype(np.uint8)):
            R = np.roll(L, -5, axis=1)
            got, want, _ = run(pkg, L, R, ws, numDisparities=D, blockSize=7, preFilterCap=cap, textureThreshold=0, uniquenessRatio=0)
            assert_same(got, want, "ws=%d cap=%d" % (ws, cap))


# ---- 5. random configurations ----------------------------------------------------------------------------------------------
def _case(rng):
    """the generator of test_gpu_dslice._case, extended by the prefilter size"""
    D = int(rng.choice([32, 48, 64, 96, 128, 192, 256, 272, 320, 512]))
    w = int(rng.choice([5, 7, 9, 11, 13, 15, 21, 25]))
    minD = int(rng.choice([0, 0, 3, -7, -20, 17]))
    W = int(rng.integers(D + abs(minD) + w + 20, D + abs(minD) + w + 200))
    H = int(rng.integers(w + 3, w + 50))
    kw = dict(numDisparities=D, blockSize=w, minDisparity=minD,
              preFilterCap=int(rng.choice([31, 31, 15, 63, 5, 1])),
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
    ws = int(rng.choice([5, 7, 9, 9, 11, 15, 21, 33, 49, 63, 75, 89, 91, 2 * int(rng.integers(2, 128)) + 1]))
    return W, H, kw, roi1, roi2, legacy, ws


@pytest.mark.parametrize("seeds", [range(0, 24), range(24, 48), range(48, 72)])
def test_random_configurations(pkg, synth, seeds):
    for seed in seeds:
        rng = np.random.default_rng(9000 + seed)
        W, H, kw, roi1, roi2, legacy, ws = _case(rng)
        L, R = synth.make_pair(synth.STREAM_SEED + 9000 + seed, W, H, kw["numDisparities"])
        if seed % 4 == 0:                       # pitched, odd-aligned views
            pad = np.zeros((H + 3, W + 37), np.uint8)
            pl, pr = pad.copy(), pad.copy()
            pl[2:2 + H, 5:5 + W] = L; pr[2:2 + H, 5:5 + W] = R
            L, R = pl[2:2 + H, 5:5 + W], pr[2:2 + H, 5:5 + W]
        got, want, _ = run(pkg, L, R, ws, roi1=roi1, roi2=roi2, legacy=legacy, **kw)
        assert_same(got, want, "seed=%d %dx%d ws=%d %s roi1=%s roi2=%s legacy=%d" % (seed, W, H, ws, kw, roi1, roi2, legacy))


# ---- 6. a live handle, batches ---------------------------------------------------------------------------------------------
def test_set_and_get_on_a_live_handle(pkg, oracle, synth):
    W, H, D, w = 400, 130, 64, 9
    kw = dict(numDisparities=D, blockSize=w)
    L, R = synth.make_pair(synth.STREAM_SEED + 8700, W, H, D)
    m = pkg.HIPMatcher(width=W, height=H, **hip_kw(kw))
    assert (m.getPreFilterType(), m.getPreFilterSize()) == (XSOBEL, 9)
    want_x = oracle.bm_compute(L, R, nthreads=8, **kw)
    assert_same(m.compute(L, R), want_x, "xsobel first")
    m.setPreFilterType(NORM)
    assert (m.getPreFilterType(), m.getPreFilterSize()) == (NORM, 9)
    assert_same(m.compute(L, R), ref.bm_compute_norm(L, R, 9, **kw), "norm 9")
    m.setPreFilterSize(21)
    assert_same(m.compute(L, R), ref.bm_compute_norm(L, R, 21, **kw), "norm 21")
    m.setPreFilterType(XSOBEL)
    assert (m.getPreFilterType(), m.getPreFilterSize()) == (XSOBEL, 21)       # the size stays, XSOBEL does not read it
    assert_same(m.compute(L, R), want_x, "xsobel again")
    # bad arguments: RTDM_ERR_BAD_PARAM, and the handle keeps what it had
    lib = pkg.binding.lib()
    for t, s in ((2, 9), (-1, 9), (NORM, 4), (NORM, 8), (NORM, 3), (NORM, 257), (XSOBEL, 10), (XSOBEL, 1), (NORM, 0), (NORM, -5)):
        assert lib.rtdm_bm_set_prefilter(m._h, t, s) == -1, (t, s)
    assert (m.getPreFilterType(), m.getPreFilterSize()) == (XSOBEL, 21)
    t = C.c_int()
    assert lib.rtdm_bm_get_prefilter(m._h, None, C.byref(t)) == -7 and lib.rtdm_bm_get_prefilter(m._h, C.byref(t), None) == -7
    for s in (5, 255):
        assert lib.rtdm_bm_set_prefilter(m._h, NORM, s) == 0
    m.close()
    with pytest.raises(pkg.binding.RtdmError) as e:
        pkg.HIPMatcher(width=W, height=H, preFilterType=NORM, preFilterSize=10)
    assert e.value.status == -1


def test_compute_device_more_frames_than_max_batch(pkg, synth):
    import torch
    n, W, H, D, ws = 5, 320, 96, 64, 9
    kw = dict(numDisparities=D, blockSize=9)
    Ls, Rs = synth.make_stream(8800, n, W, H, D)
    dL, dR = torch.from_numpy(Ls).cuda(), torch.from_numpy(Rs).cuda()
    dD = torch.zeros((n, H, W), dtype=torch.int16, device="cuda")
    m = pkg.HIPMatcher(width=W, height=H, max_batch=2, preFilterType=NORM, preFilterSize=ws, **hip_kw(kw))
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        m.compute_device(dL, dR, dD, s.cuda_stream)
    s.synchronize()
    m.close()
    got = dD.cpu().numpy()
    for i in range(n):
        assert_same(got[i], ref.bm_compute_norm(Ls[i], Rs[i], ws, **kw), "frame %d" % i)


def test_compute_batch_page_locked_and_pageable(pkg, synth):
    import torch
    n, W, H, D, ws = 4, 336, 80, 48, 11
    kw = dict(numDisparities=D, blockSize=9)
    Ls, Rs = synth.make_stream(8900, n, W, H, D)
    pl, pr = torch.from_numpy(Ls).pin_memory(), torch.from_numpy(Rs).pin_memory()
    po = torch.full((n, H, W), 12345, dtype=torch.int16).pin_memory()
    m = pkg.HIPMatcher(width=W, height=H, max_batch=2, preFilterType=NORM, preFilterSize=ws, **hip_kw(kw))
    got = m.compute_batch(pl.numpy(), pr.numpy(), po.numpy())
    again = m.compute_batch(Ls, Rs)
    m.close()
    assert np.array_equal(got, again)
    for i in range(n):
        assert_same(got[i], ref.bm_compute_norm(Ls[i], Rs[i], ws, **kw), "frame %d" % i)


# ---- 7. the chains ---------------------------------------------------------------------------------------------------------
Q_TEST = np.array([[1, 0, 0, -320.3], [0, 1, 0, -36.8], [0, 0, 0, 700.25], [0, 0, 1 / 12.0, 0.0]])


def test_compute_depth(pkg, oracle, synth):
    W, H, D, ws = 400, 120, 64, 9
    kw = dict(numDisparities=D, blockSize=9)
    L, R = synth.make_pair(synth.STREAM_SEED + 8950, W, H, D)
    mask = ((L > 100) * 255).astype(np.uint8)
    regions = [(130, 8, 200, 80), (0, 0, W, H), (300, 30, 60, 20)]
    m = pkg.HIPMatcher(width=W, height=H, preFilterType=NORM, preFilterSize=ws, **hip_kw(kw))
    mean, cnt, disp = m.compute_depth(L, R, Q_TEST, mask, regions, calibration_unit=25.0, want_disp=True)
    m.close()
    want_disp = ref.bm_compute_norm(L, R, ws, **kw)
    assert_same(disp, want_disp)
    wm, wc = oracle.depth_stats(want_disp, Q_TEST, mask, regions, 25.0)
    assert np.array_equal(cnt, wc) and wc[1] > 1000
    assert np.allclose(mean, wm, rtol=1e-9, atol=0)


def test_raw_frames_to_disparity_in_one_call(pkg, oracle, synth):
    res, D, w, ws = "320x240", 32, 7, 9
    c, maps = ru.maps(oracle, res)
    left, right = ru.rgb_pair(synth, 2, c["W"], c["H"])
    x, y, rw, rh = c["roi"]
    r = pkg.HIPRectifier(*maps, roi=c["roi"])
    m = pkg.HIPMatcher(numOfDisparities=D, blockSize=w, width=rw, height=rh, preFilterType=NORM, preFilterSize=ws)
    gl = oracle.rectify_gray(left, maps[0], maps[1], c["roi"]); gr = oracle.rectify_gray(right, maps[2], maps[3], c["roi"])
    assert_same(r.compute(m, left, right), ref.bm_compute_norm(gl, gr, ws, numDisparities=D, blockSize=w))
    m.close(); r.close()


def test_whole_frame_chain(pkg, oracle, synth):
    res, D, w, ws = "320x240", 32, 7, 11
    c, maps = ru.maps(oracle, res)
    left, right = ru.red_scene(synth, 1, c["W"], c["H"], D)
    x, y, rw, rh = c["roi"]
    rect = pkg.HIPRectifier(*maps, roi=c["roi"])
    m = pkg.HIPMatcher(numOfDisparities=D, blockSize=w, width=rw, height=rh, preFilterType=NORM, preFilterSize=ws)
    det = pkg.HIPObjectDetector(rw, rh)
    boxes, mean, cnt, disp = pkg.estimate_frame(m, rect, det, left, right, c["Q"], min_area=40, want_disp=True)
    gl = oracle.rectify_gray(left, maps[0], maps[1], c["roi"]); gr = oracle.rectify_gray(right, maps[2], maps[3], c["roi"])
    col = oracle.rectify_rgb(left, maps[0], maps[1], c["roi"])
    fout = oracle.morph_open_close(oracle.hsv_inrange(col, oracle.HSV_LOW, oracle.HSV_HIGH))
    want_boxes = oracle.external_boxes(fout, 40, True)
    assert len(want_boxes) >= 2 and boxes == want_boxes[:64]
    want_disp = ref.bm_compute_norm(gl, gr, ws, numDisparities=D, blockSize=w, roi1=oracle.union_box(want_boxes))
    assert_same(disp, want_disp)
    wm, wc = oracle.depth_stats(want_disp, c["Q"], fout, want_boxes[:64])
    assert np.array_equal(cnt, wc) and np.allclose(mean, wm, rtol=1e-9, atol=0)
    det.close(); m.close(); rect.close()


def test_compute_filtered_with_a_right_matcher(pkg, synth):
    W, H, D, w, ws = 320, 180, 64, 9, 15
    L, R = synth.make_pair(synth.STREAM_SEED + 8960, W, H, D)
    m = pkg.HIPMatcher(numOfDisparities=D, blockSize=w, width=W, height=H, preFilterType=NORM, preFilterSize=ws)
    rm = pkg.create_right_matcher(m)
    assert (rm.getPreFilterType(), rm.getPreFilterSize()) == (NORM, ws)        # W1: createRightMatcher copies both
    f = pkg.create_disparity_wls_filter(m)
    got, raw = f.compute_filtered(m, rm, L, R, want_raw=True)
    dL = m.compute(L, R)
    assert_same(raw, dL)
    assert_same(dL, ref.bm_compute_norm(L, R, ws, numDisparities=D, blockSize=w))
    dR = rm.compute(R, L)
    assert_same(dR, ref.bm_compute_norm(R, L, ws, numDisparities=D, blockSize=w, minDisparity=-(0 + D) + 1, textureThreshold=0,
                                        uniquenessRatio=0, speckleWindowSize=0, disp12MaxDiff=1000000))
    assert_same(got, f.filter(dL, L, None, dR))
    f.close(); rm.close(); m.close()


# ---- 8. the frame fill as a launch of its own ---------------------------------------------------------------------------------
_CHILD = r'''
import sys, zlib
sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np
import torch
assert torch.cuda.is_available()
from conftest import load
import bm_norm_ref as ref
pkg = load(); synth = pkg.synth
for (W, H, D, w, ws, roi) in [(320, 100, 64, 9, 9, None), (333, 77, 32, 7, 21, (100, 10, 150, 50)), (640, 120, 64, 13, 5, None)]:
    L, R = synth.make_pair(synth.STREAM_SEED + 8990 + W, W, H, D)
    m = pkg.HIPMatcher(numOfDisparities=D, blockSize=w, width=W, height=H, preFilterType=0, preFilterSize=ws)
    if roi: m.setROI1(roi)
    got = m.compute(L, R)
    m.close()
    want = ref.bm_compute_norm(L, R, ws, numDisparities=D, blockSize=w, roi1=roi)
    assert np.array_equal(got, want), (W, H, D, w, ws, int((got != want).sum()))
    print("CRC", W, H, ws, zlib.crc32(got.tobytes()))
print("ok")
'''


def test_fill_in_prefilter_switch_changes_nothing():
    outs = {}
    for flag in ("1", "0"):
        p = subprocess.run([sys.executable, "-c", _CHILD % (ROOT, os.path.join(ROOT, "tests"))], stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, text=True, timeout=600, env=dict(os.environ, RTDM_FILL_IN_PREFILTER=flag))
        assert p.returncode == 0 and p.stdout.strip().endswith("ok"), p.stderr[-3000:]
        outs[flag] = [ln for ln in p.stdout.splitlines() if ln.startswith("CRC")]
    assert outs["1"] == outs["0"] and len(outs["1"]) == 3
