"""StereoSGBM with numDisparities above 256: the wide-line path pass (k_sgm_wide.hip), one wave per line up to 1024
disparities and four waves per line above.  Every result is compared bit for bit with the oracle (oracle/sgm_oracle.c).
rtdm_debug_sgm_wide_paths forces the wide pass, in either form, on any numDisparities, so that lane and wave boundaries can
be put anywhere and both forms can be held against the narrow kernels; it is reset in `finally` everywhere."""
import contextlib
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, load

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    import torch                         # torch first: it brings its own HIP runtime and must initialise before ours
    assert torch.cuda.is_available(), "the -m gpu suite needs an MI355X"
    return load()


@contextlib.contextmanager
def forced_wide(pkg, mode):
    pkg.binding.lib().rtdm_debug_sgm_wide_paths(mode)
    try:
        yield
    finally:
        pkg.binding.lib().rtdm_debug_sgm_wide_paths(0)


def assert_same(got, want, what=""):
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError("%s: %d / %d pixels differ; first at (y,x)=%s got %d want %d" % (
            what, len(bad), got.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])]))


def run(pkg, L, R, **kw):
    """-> (device result, path variant, sweeps)"""
    H, W = L.shape
    kw = dict(kw)
    kw["numOfDisparities"] = kw.pop("numDisparities")
    m = pkg.HIPSemiGlobalMatcher(width=W, height=H, **kw)
    try:
        got = m.compute(L, R)
        return got, m.path_variant, m.pass_stats()[0]
    finally:
        m.close()


def shifted_pair(seed, W, H, shift):
    """A textured pair whose right view is the left one moved by `shift` columns: L[x] = R[x - shift]."""
    rng = np.random.default_rng(seed)
    T = rng.integers(0, 256, (H, W + shift)).astype(np.float64)
    T = (T + np.roll(T, 1, 1) + np.roll(T, -1, 1) + np.roll(T, 1, 0) + np.roll(T, -1, 0)) / 5
    T = T.astype(np.uint8)
    return T[:, :W].copy(), T[:, shift:shift + W].copy()


# ---- 1. numDisparities > 256 on synthetic pairs, both modes ------------------------------------------------------------------
@pytest.mark.parametrize("paths", [5, 8])
@pytest.mark.parametrize("D,W,H", [(272, 480, 60), (320, 560, 40), (384, 640, 80), (512, 780, 48), (1024, 1300, 40)])
def test_more_than_256_disparities(pkg, oracle, synth, D, W, H, paths):
    L, R = synth.make_pair(synth.STREAM_SEED + 8000 + D + paths, W, H, min(D, 200))
    got, variant, sweeps = run(pkg, L, R, numDisparities=D, paths=paths)
    want = oracle.sgm_compute(L, R, numDisparities=D, paths=paths)
    assert variant == ("wide_w1" if D <= 1024 else "wide_w4"), variant
    assert sweeps == 0
    assert_same(got, want, "D=%d paths=%d" % (D, paths))
    assert (want != -16).mean() > 0.05


# ---- 2. extremes of numDisparities / minDisparity ----------------------------------------------------------------------------
@pytest.mark.parametrize("D,minD,W,H", [(2048, -1024, 2348, 40), (4080, -2033, 4096, 24), (512, 300, 1100, 48),
                                        (320, -17, 600, 40), (1040, -3, 1300, 30)])
def test_extreme_disparity_ranges(pkg, oracle, synth, D, minD, W, H):
    L, R = synth.make_pair(synth.STREAM_SEED + 8100 + D + minD, W, H, 200)
    got, variant, _ = run(pkg, L, R, numDisparities=D, minDisparity=minD)
    want = oracle.sgm_compute(L, R, numDisparities=D, minDisparity=minD)
    assert variant.startswith("wide"), variant
    assert_same(got, want, "D=%d minD=%d" % (D, minD))


def test_empty_domain_is_all_invalid(pkg, oracle, synth):
    # W1 <= 0 for every frame the handle takes (no volumes at all), and for a frame narrower than the handle's maximum
    L, R = synth.make_pair(synth.STREAM_SEED + 8150, 500, 30, 64)
    got, _, _ = run(pkg, L, R, numDisparities=512)
    assert (got == -16).all()
    assert_same(got, oracle.sgm_compute(L, R, numDisparities=512))
    m = pkg.HIPSemiGlobalMatcher(numOfDisparities=512, minDisparity=-100, width=900, height=30)
    try:
        got = m.compute(L, R)                           # 500 - 100 - 412 = -12 columns
        assert_same(got, oracle.sgm_compute(L, R, numDisparities=512, minDisparity=-100))
        assert (got == -101 * 16).all()
        L2, R2 = synth.make_pair(synth.STREAM_SEED + 8151, 900, 30, 200)
        assert_same(m.compute(L2, R2), oracle.sgm_compute(L2, R2, numDisparities=512, minDisparity=-100))
    finally:
        m.close()


# ---- 3. known answer above 255 --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("paths", [5, 8])
def test_shift_of_300_columns_is_found(pkg, oracle, paths):
    # an 8-bit winner key would return 300 & 0xff = 44
    W, H = 640, 40
    L, R = shifted_pair(300 + paths, W, H, 300)
    got, variant, _ = run(pkg, L, R, numDisparities=320, paths=paths)
    assert variant == "wide_w1"
    assert_same(got, oracle.sgm_compute(L, R, numDisparities=320, paths=paths))
    inner = got[4:-4, 324:W - 4]
    assert (inner == 300 * 16).mean() > 0.95, np.unique(inner, return_counts=True)


# ---- 4. windows, the cost check, coercions ----------------------------------------------------------------------------------
@pytest.mark.parametrize("bs", [1, 3, 7, 9, 19])
def test_windows(pkg, oracle, synth, bs):
    L, R = synth.make_pair(synth.STREAM_SEED + 8200 + bs, 420, 50, 200)
    got, _, _ = run(pkg, L, R, numDisparities=272, blockSize=bs, paths=8)
    assert_same(got, oracle.sgm_compute(L, R, numDisparities=272, blockSize=bs, paths=8), "bs=%d" % bs)


def test_frame_whose_costs_would_wrap_is_refused_and_the_handle_goes_on(pkg, oracle, synth):
    D, W, H = 272, 380, 40
    Lo, Ro = np.full((H, W), 255, np.uint8), np.zeros((H, W), np.uint8)
    m = pkg.HIPSemiGlobalMatcher(blockSize=25, numOfDisparities=D, width=W, height=H, paths=8)
    try:
        with pytest.raises(Exception):
            m.compute(Lo, Ro)
        with pytest.raises(ValueError):
            oracle.sgm_compute(Lo, Ro, numDisparities=D, blockSize=25)
        L, R = synth.make_pair(synth.STREAM_SEED + 8250, W, H, 200)
        assert_same(m.compute(L, R), oracle.sgm_compute(L, R, numDisparities=D, blockSize=25))
    finally:
        m.close()


@pytest.mark.parametrize("kw", [dict(P1=0, P2=0), dict(P1=-5, P2=3), dict(P1=900, P2=100), dict(uniquenessRatio=0),
                                dict(uniquenessRatio=100), dict(uniquenessRatio=-1), dict(disp12MaxDiff=0),
                                dict(disp12MaxDiff=-3), dict(speckleWindowSize=0), dict(speckleWindowSize=300, speckleRange=1),
                                dict(P2=32000, blockSize=1, paths=8), dict(P2=32000, blockSize=1, paths=5)])
def test_parameters(pkg, oracle, synth, kw):
    L, R = synth.make_pair(synth.STREAM_SEED + 8300 + len(repr(kw)), 460, 44, 200)
    got, _, _ = run(pkg, L, R, numDisparities=336, **kw)
    assert_same(got, oracle.sgm_compute(L, R, numDisparities=336, **kw), repr(kw))


def test_every_cost_saturated_is_no_winner(pkg, oracle, synth):
    W, H, D = 400, 50, 288
    kw = dict(blockSize=11, uniquenessRatio=0, speckleWindowSize=20, speckleRange=2, P1=600, P2=20000, paths=8)
    Ls, Rs = synth.make_stream(155, 1, W, H, 200)
    L, R = (Ls[0] // 32 * 32).astype(np.uint8), (Rs[0] // 32 * 32).astype(np.uint8)
    for mode in (0, 4):
        with forced_wide(pkg, mode):
            got, _, _ = run(pkg, L, R, numDisparities=D, **kw)
        assert_same(got, oracle.sgm_compute(L, R, numDisparities=D, **kw), "mode %d" % mode)


# ---- 5. entry points -----------------------------------------------------------------------------------------------------------
def test_pitched_host_views(pkg, oracle, synth):
    W, H, D = 500, 40, 288
    L, R = synth.make_pair(synth.STREAM_SEED + 8400, W, H, 200)
    bigL = np.zeros((H, W + 37), np.uint8); bigL[:, 5:5 + W] = L
    bigR = np.zeros((H, W + 61), np.uint8); bigR[:, 11:11 + W] = R
    vL, vR = bigL[:, 5:5 + W], bigR[:, 11:11 + W]
    assert not vL.flags.c_contiguous and not vR.flags.c_contiguous
    got, _, _ = run(pkg, vL, vR, numDisparities=D)
    assert_same(got, oracle.sgm_compute(L, R, numDisparities=D))


@pytest.mark.parametrize("D,paths", [(272, 8), (1040, 5)])
def test_compute_device_more_frames_than_max_batch(pkg, oracle, synth, D, paths):
    import torch
    n, W, H = 5, D + 220, 36
    Ls, Rs = synth.make_stream(8500 + D, n, W, H, 200)
    m = pkg.HIPSemiGlobalMatcher(numOfDisparities=D, width=W, height=H, max_batch=2, paths=paths)
    try:
        dL, dR = torch.from_numpy(Ls).cuda(), torch.from_numpy(Rs).cuda()
        dD = torch.zeros((n, H, W), dtype=torch.int16, device="cuda")
        m.compute_device(dL, dR, dD, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        got = dD.cpu().numpy()
        for i in range(n):
            assert_same(got[i], m.compute(Ls[i], Rs[i]), "frame %d vs a single call" % i)
            assert_same(got[i], oracle.sgm_compute(Ls[i], Rs[i], numDisparities=D, paths=paths), "frame %d" % i)
    finally:
        m.close()


# ---- 6. both wide forms held against the narrow kernels and against each other -------------------------------------------------
@pytest.mark.parametrize("D", [16, 48, 64, 128, 256])
def test_forced_wide_equals_narrow_kernels(pkg, oracle, synth, D):
    for paths, W, H in ((8, D + 61, 23), (5, D + 44, 18)):
        L, R = synth.make_pair(synth.STREAM_SEED + 8600 + D + paths, W, H, D)
        kw = dict(numDisparities=D, paths=paths, P1=600 if D % 32 else 37, P2=2400 if D % 48 else 30000)
        base, v0, _ = run(pkg, L, R, **kw)
        assert not v0.startswith("wide"), v0
        assert_same(base, oracle.sgm_compute(L, R, **kw), "narrow D=%d" % D)
        for mode, name in ((1, "wide_w1"), (4, "wide_w4")):
            with forced_wide(pkg, mode):
                got, variant, sweeps = run(pkg, L, R, **kw)
            assert variant == name and sweeps == 0, (variant, sweeps)
            assert_same(got, base, "D=%d paths=%d %s" % (D, paths, name))


@pytest.mark.parametrize("D,mode_a,mode_b", [(272, 1, 4), (1024, 1, 4), (1040, 0, 4)])
def test_both_wide_forms_agree(pkg, oracle, synth, D, mode_a, mode_b):
    # 272: one wave of 34 live lanes (8 disparities each) against 136 live lanes over three waves (2 each); 1024: a full wave of
    # 16 per lane against 256 lanes of 4; 1040: the four-wave form with a partly live third wave (the one-wave form holds at most
    # 1024, so mode 1 runs four waves there as well)
    W, H = D + 230, 30
    L, R = synth.make_pair(synth.STREAM_SEED + 8700 + D, W, H, 200)
    want = oracle.sgm_compute(L, R, numDisparities=D, minDisparity=-5, uniquenessRatio=3)
    outs = []
    for mode in (mode_a, mode_b):
        with forced_wide(pkg, mode):
            got, variant, _ = run(pkg, L, R, numDisparities=D, minDisparity=-5, uniquenessRatio=3)
        assert variant == ("wide_w1" if mode == 1 or (mode == 0 and D <= 1024) else "wide_w4"), (mode, variant)
        assert_same(got, want, "D=%d mode %d" % (D, mode))
        outs.append(got)
    assert_same(outs[0], outs[1])


# ---- 7. the A/B environment switches never send D > 256 to a narrow kernel ------------------------------------------------------
_AB_CASE = r'''
import sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import numpy as np
import torch
from conftest import load
from oracle import oracle as orc
pkg = load(); syn = load("synth")
orc.build()
D, W, H = 512, 760, 40
L, R = syn.make_pair(syn.STREAM_SEED + 8800, W, H, 200)
for paths in (5, 8):
    m = pkg.HIPSemiGlobalMatcher(numOfDisparities=D, width=W, height=H, paths=paths)
    got = m.compute(L, R)
    v, sw = m.path_variant, m.pass_stats()[0]
    m.close()
    assert v == "wide_w1" and sw == 0, (v, sw)
    assert np.array_equal(got, orc.sgm_compute(L, R, numDisparities=D, paths=paths)), paths
print("ok")
'''


@pytest.mark.parametrize("var", ["RTDM_SGM_SWEEP", "RTDM_SGM_DUAL"])
def test_ab_switches_leave_wide_lines_alone(var):
    env = dict(os.environ, **{var: "0"})
    p = subprocess.run(["timeout", "-k", "10", "600", sys.executable, "-c", _AB_CASE % (ROOT, os.path.join(ROOT, "tests"))],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=660, env=env)
    assert p.returncode == 0 and p.stdout.strip().endswith("ok"), (var, p.returncode, p.stdout[-500:], p.stderr[-3000:])


# ---- 8. dispatch and allocation ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("paths,W,H,D", [(8, 300, 90, 64), (5, 130, 40, 96), (8, 233, 61, 128)])
def test_narrow_configurations_keep_their_kernels(pkg, oracle, synth, paths, W, H, D):
    # the configurations test_gpu_round3.py pins the row-synchronous sweeps on
    L, R = synth.make_pair(synth.STREAM_SEED + 8900 + D, W, H, D)
    got, variant, sweeps = run(pkg, L, R, numDisparities=D, paths=paths)
    assert variant == "sweep" and sweeps == (2 if paths == 8 else 1), (variant, sweeps)
    assert_same(got, oracle.sgm_compute(L, R, numDisparities=D, paths=paths))


def test_volumes_are_sized_on_the_domain(pkg):
    # 4096 x 2160, D = 4080: 16 domain columns -> about 1 GB in all; sized on max_width it would be ~250 GB
    import ctypes as C
    B = pkg.binding
    p = B.SGMParams(5, 0, 4080, 600, 2400, 10, 100, 32, 1, 8)
    h = C.c_void_p()
    assert B.lib().rtdm_sgm_create(C.byref(p), 4096, 2160, 1, 0, C.byref(h)) == 0, B.lib().rtdm_last_hip_error()
    assert B.lib().rtdm_sgm_path_variant(h) == b""
    B.lib().rtdm_sgm_destroy(h)
    # still refused: frames wider than 4096, windows above 255, P2 above 32000
    for args, width in (((5, 0, 512, 600, 2400), 4097), ((257, 0, 512, 600, 2400), 1024), ((5, 0, 512, 600, 32001), 1024)):
        p = B.SGMParams(*args, 10, 100, 32, 1, 8)
        assert B.lib().rtdm_sgm_create(C.byref(p), width, 64, 1, 0, C.byref(h)) == -6, (args, width)      # RTDM_ERR_UNSUPPORTED
