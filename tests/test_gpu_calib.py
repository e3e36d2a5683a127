"""GPU tests of the rectification built from the calibration files: the map kernel (k_rectmap.hip) bit for bit against
orc_init_undistort_rectify_map, the handle rtdm_rectify_create_calib builds against one made from oracle maps, and
HIPRectifier.from_calibration against the oracle chain.  Inputs: tests/golden/calib.json and tests/golden/calib_yml/ only."""
import ctypes as C

import numpy as np
import pytest

import calib_hostbuild as hb
import calib_ref as cr
import rectify_util as ru
from calib_ref import check_rectification, tie_calibration

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    import torch                         # torch first: it brings its own HIP runtime and must initialise before ours
    assert torch.cuda.is_available()
    from conftest import load
    return load()


def assert_maps_equal(got, want, where):
    assert got[0].dtype == np.int16 and got[1].dtype == np.uint16 and got[0].shape == want[0].shape and got[1].shape == want[1].shape
    bad1, bad2 = int((got[0] != want[0]).any(-1).sum()), int((got[1] != want[1]).sum())
    assert bad1 == 0 and bad2 == 0, "%s: %d map1 and %d map2 entries differ" % (where, bad1, bad2)


# ---- 1. the map kernel against the oracle --------------------------------------------------------------------------------
@pytest.mark.parametrize("res, cams", [("320x240", "12"), ("640x480", "12"), ("1280x720", "1")])
def test_maps_of_the_recorded_calibrations(pkg, oracle, res, cams):
    c = ru.calib(res)
    for k in cams:
        a = (c["M" + k], c["D" + k], c["R" + k], c["P" + k], c["W"], c["H"])
        assert_maps_equal(pkg.init_undistort_rectify_map(*a), oracle.init_undistort_rectify_map(*a), res + " camera " + k)


@pytest.mark.parametrize("H", [1, 3])
@pytest.mark.parametrize("W", [1, 63, 64, 65, 129, 321])
def test_maps_at_every_checkpoint_boundary(pkg, oracle, W, H):
    c = ru.calib("320x240")
    a = (c["M1"], c["D1"], c["R1"], c["P1"], W, H)
    assert_maps_equal(pkg.init_undistort_rectify_map(*a), oracle.init_undistort_rectify_map(*a), "%dx%d" % (W, H))
    # every exact coordinate of this camera is a tie of rint(u * 32): the last bits of the accumulated ray decide the entry
    t = tie_calibration() + (W, H)
    assert_maps_equal(pkg.init_undistort_rectify_map(*t), oracle.init_undistort_rectify_map(*t), "ties %dx%d" % (W, H))


def test_maps_where_a_directly_computed_ray_is_wrong(pkg, oracle):
    # on the recorded calibrations x0 + j * ir[0] happens to give the same maps as the accumulated ray; on this set it does not
    # (test_calib_cpu.py shows both on the CPU), so a kernel that dropped the row accumulation fails here
    M, D, R, P = tie_calibration()
    W, H = 640, 480
    want = oracle.init_undistort_rectify_map(M, D, R, P, W, H)
    direct = cr.rect_map(M, D, R, P, W, H, accumulate=False)
    assert (direct[1] != want[1]).sum() > 100
    assert_maps_equal(pkg.init_undistort_rectify_map(M, D, R, P, W, H), want, "ties 640x480")


def test_maps_with_all_twelve_coefficients(pkg, oracle):
    c = ru.calib("320x240")
    D = np.array([-0.21, 0.07, 1.1e-3, -0.8e-3, -0.012, 0.02, -0.011, 0.004, 1.5e-3, -0.7e-3, 0.9e-3, 1.2e-3, 0, 0])
    M = np.array([[88.3, 0, 47.2], [0, 86.9, 33.4], [0, 0, 1.0]])
    P = np.array([[61.0, 0, 50.1, 0], [0, 61.0, 30.7, 0], [0, 0, 1.0, 0]])
    a = (M, D, c["R2"], P, 97, 65)
    got, want = pkg.init_undistort_rectify_map(*a), oracle.init_undistort_rectify_map(*a)
    assert_maps_equal(got, want, "12 coefficients 97x65")
    assert not np.array_equal(want[1], oracle.init_undistort_rectify_map(M, D[:8], c["R2"], P, 97, 65)[1])   # s1..s4 matter here


def test_device_form_and_run_to_run(pkg, oracle):
    import torch
    L = pkg.binding.lib()
    c = ru.calib("640x480")
    W, H = c["W"], c["H"]
    a = [np.ascontiguousarray(c[k], np.float64).reshape(-1) for k in ("M2", "D2", "R2", "P2")]
    want = oracle.init_undistort_rectify_map(c["M2"], c["D2"], c["R2"], c["P2"], W, H)
    s = torch.cuda.Stream()
    runs = []
    for stream in (None, s.cuda_stream):
        m1 = torch.zeros((H, W, 2), dtype=torch.int16, device="cuda")
        m2 = torch.zeros((H, W), dtype=torch.int16, device="cuda")      # the uint16 bits, in torch's 16-bit integer type
        torch.cuda.synchronize()
        st = L.rtdm_undistort_rectify_map_device(*[v.ctypes.data for v in a], W, H, 0, m1.data_ptr(), m2.data_ptr(), stream)
        assert st == 0
        runs.append((m1.cpu().numpy(), m2.cpu().numpy().view(np.uint16)))
        assert_maps_equal(runs[-1], want, "device form")
    assert_maps_equal(runs[0], runs[1], "two builds")
    assert_maps_equal(pkg.init_undistort_rectify_map(c["M2"], c["D2"], c["R2"], c["P2"], W, H), runs[0], "host form again")
    # a misaligned map1 is refused, not written
    assert L.rtdm_undistort_rectify_map_device(*[v.ctypes.data for v in a], W, H, 0, m1.data_ptr() + 2, m2.data_ptr(), None) == -2


# ---- 2. handle equivalence -------------------------------------------------------------------------------------------------
def _rectification_320(pkg):
    cal = pkg.load_calibration(hb.yml("320x240", "intrinsics"), hb.yml("320x240", "extrinsics"))
    return cal, pkg.stereo_rectify(cal, alpha=-1.0)


def test_handle_from_calibration_equals_handle_from_oracle_maps(pkg, oracle, synth):
    B = pkg.binding
    L = B.lib()
    cal, rect = _rectification_320(pkg)
    W, H, roi = 320, 240, (49, 46, 233, 156)
    maps = oracle.init_undistort_rectify_map(cal.M1, cal.D1, rect["R1"], rect["P1"], W, H) + \
        oracle.init_undistort_rectify_map(cal.M2, cal.D2, rect["R2"], rect["P2"], W, H)
    a = pkg.HIPRectifier(*maps, roi=roi, max_batch=2)
    b = pkg.HIPRectifier.__new__(pkg.HIPRectifier)
    b.width, b.height, b.roi, b._h = W, H, roi, C.c_void_p()
    B.check(L.rtdm_rectify_create_calib(C.byref(cal._c), C.byref(rect["_c"]), *roi, 2, 0, C.byref(b._h)), "rtdm_rectify_create_calib")
    left, right = ru.rgb_pair(synth, 3, W, H)
    ga, gb = a.gray(left, right), b.gray(left, right)
    assert np.array_equal(ga[0], gb[0]) and np.array_equal(ga[1], gb[1])
    assert ga[0].shape == (156, 233) and ga[0].std() > 1
    for which, frame in ((0, left), (1, right)):
        assert np.array_equal(a.rgb(frame, which), b.rgb(frame, which))
    assert np.array_equal(ga[0], oracle.rectify_gray(left, maps[0], maps[1], roi))
    a.close(); b.close()


# ---- 3. HIPRectifier.from_calibration ----------------------------------------------------------------------------------------
def test_from_calibration_reproduces_the_oracle_chain(pkg, oracle, synth):
    res = "320x240"
    intr, extr = hb.yml(res, "intrinsics"), hb.yml(res, "extrinsics")
    c = ru.calib(res)
    r = pkg.HIPRectifier.from_calibration(intr, extr, max_batch=2)
    assert r.roi == c["roi"] == (49, 46, 233, 156) and (r.width, r.height) == (320, 240)
    cal, rect = _rectification_320(pkg)
    assert np.array_equal(r.Q, rect["Q"]) and r.Q.shape == (4, 4)
    ref = cr.stereo_rectify(cal.M1, cal.D1, cal.M2, cal.D2, cal.R, cal.T, 320, 240, cr.ZERO_DISPARITY, -1.0)
    check_rectification(r.rectification, ref, "from_calibration")
    maps = oracle.init_undistort_rectify_map(cal.M1, cal.D1, rect["R1"], rect["P1"], 320, 240) + \
        oracle.init_undistort_rectify_map(cal.M2, cal.D2, rect["R2"], rect["P2"], 320, 240)
    left, right = ru.rgb_pair(synth, 4, 320, 240)
    gl, gr = r.gray(left, right)
    assert np.array_equal(gl, oracle.rectify_gray(left, maps[0], maps[1], r.roi))
    assert np.array_equal(gr, oracle.rectify_gray(right, maps[2], maps[3], r.roi))
    assert np.array_equal(r.rgb(left, 0), oracle.rectify_rgb(left, maps[0], maps[1], r.roi))
    # the handle drives the matcher to the same disparity as a handle made from maps
    x, y, rw, rh = r.roi
    m = pkg.HIPMatcher(numOfDisparities=32, blockSize=7, width=rw, height=rh, max_batch=2)
    from_maps = pkg.HIPRectifier(*maps, roi=r.roi, max_batch=2)
    d = r.compute(m, left, right)
    assert np.array_equal(d, from_maps.compute(m, left, right))
    assert np.array_equal(d, oracle.bm_compute(gl, gr, numDisparities=32, blockSize=7, nthreads=8))
    # roi="rectify": the computed ROIs, by the reference's rule
    rr = pkg.HIPRectifier.from_calibration(intr, extr, roi="rectify")
    r1, r2 = ref["ROI1"], ref["ROI2"]
    assert rr.roi == (max(r1[0], r2[0]), max(r1[1], r2[1]), min(r1[2], r2[2]), min(r1[3], r2[3]))
    assert rr.rectification["ROI1"] == tuple(r1) and rr.rectification["ROI2"] == tuple(r2)
    g2 = rr.gray(left, right)[0]
    assert np.array_equal(g2, oracle.rectify_gray(left, maps[0], maps[1], rr.roi))
    m.close(); from_maps.close(); rr.close(); r.close()
