"""StereoSGBM's census pixel cost (rtdm_sgm_set_cost, rules N1-N5 of DESIGN.md section 4.20) on the device: every result is
compared bit for bit with sgm_census_ref.sgm_compute -- N1 and N2 in NumPy, every later stage through the C oracle's own entry
points (sgm_hh4_ref's recurrence for four paths).  Tolerance 0.  The cost is the project's own: there is no library to be at
parity with, and what it gains on real pairs with unequal exposure is unmeasured; what is shown here is that the device computes
the stated rules on every route of the cost stage, and the invariance N1 promises.

The inputs (sgm_census_cases.py) are checked on the CPU in test_sgm_census_cpu.py: textured cases are at least 30 % valid in
the reference, the checked-route pair is not refused, the refusal pair is."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import sgm_census_cases as cases
import sgm_census_ref as ref
import sgm_cn_ref
from conftest import load

pytestmark = pytest.mark.gpu


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


def matcher(pkg, W, H, census=None, max_batch=1, cap=0, **kw):
    """a HIPSemiGlobalMatcher from the reference's parameter names; census: (cw, ch), or None for the BT cost"""
    M = pkg.HIPSemiGlobalMatcher
    kw = dict(kw)
    kw["numOfDisparities"] = kw.pop("numDisparities")
    cost = dict(cost=M.COST_CENSUS, census=census) if census else {}
    return M(width=W, height=H, max_batch=max_batch, preFilterCap=cap, **dict(kw, **cost))


def device_call(pkg, m, Ls, Rs, pad_cols=0, pad_rows=0):
    """rtdm_sgm_compute_device on n frames held in planes with `pad_cols` spare columns per row and `pad_rows` spare rows per
    frame, both filled with values the call must not read into the result -> (status, int16 [n, H, W])"""
    import torch
    n, H, W = Ls.shape
    rng = np.random.default_rng(5)

    def plane(a):
        p = rng.integers(0, 256, (n, H + pad_rows, W + pad_cols)).astype(np.uint8)
        p[:, :H, :W] = a
        return torch.from_numpy(p).cuda()
    dL, dR = plane(Ls), plane(Rs)
    dD = torch.full((n, H, W), 12345, dtype=torch.int16, device="cuda")
    pitch = W + pad_cols
    rc = pkg.binding.lib().rtdm_sgm_compute_device(m._h, n, dL.data_ptr(), dR.data_ptr(), pitch, pitch * (H + pad_rows), W, H,
                                                   dD.data_ptr(), W * 2, W * H * 2, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, dD.cpu().numpy()


# ---- 1. every route of the cost stage ---------------------------------------------------------------------------------------------
VARIANT = {4: ("vert",), 5: ("sweep", "half"), 8: ("sweep", "half")}       # the path passes are not what is under test here


@pytest.mark.parametrize("i", range(len(cases.ROUTES)), ids=[cases.case_id(c) for c in cases.ROUTES])
def test_routes(pkg, i):
    c = cases.ROUTES[i]
    W, H, D, minD, bs, paths, census, n, P2 = c
    Ls, Rs = cases.case_frames(i, c)
    kw = cases.params(c)
    want = [ref.sgm_compute(Ls[f], Rs[f], census=census, **kw) for f in range(n)]
    for f in range(n):
        share = cases.valid_share(want[f], c)
        assert share >= 0.30, "the reference's map is %.3f valid: parity on it would show nothing" % share
    m = matcher(pkg, W, H, census, max_batch=min(n, 2), **kw)
    try:
        assert m.getCost() == (m.COST_CENSUS, census)
        if n == 1 and i % 2 == 0:
            got = m.compute(Ls[0], Rs[0])[None]                                   # the host entry point
        else:
            rc, got = device_call(pkg, m, Ls, Rs, pad_cols=31 if n > 1 else 0, pad_rows=3 if n == 3 else 0)
            assert rc == 0
        variant = m.path_variant
    finally:
        m.close()
    for f in range(n):
        assert_same(got[f], want[f], "%s frame %d" % (cases.case_id(c), f))
    assert variant in (("wide_w1",) if D > 256 else VARIANT[paths])
    assert n == 1 or len({g.tobytes() for g in got}) == n


def test_noise_pair(pkg):
    c = cases.NOISE_CASE
    W, H, D, minD, bs, paths, census, n, P2 = c
    L, R = cases.noise_pair(9250, W, H)
    kw = cases.params(c)
    m = matcher(pkg, W, H, census, **kw)
    try:
        assert_same(m.compute(L, R), ref.sgm_compute(L, R, census=census, **kw), "noise")
    finally:
        m.close()


@pytest.mark.parametrize("cw,ch", cases.WINDOWS)
def test_every_window(pkg, cw, ch):
    """all twelve descriptor kernels, on a frame that is no multiple of their 64 x 16 tile, with many ties (values 0 .. 7)"""
    W, H, D = 16 + 67, 19, 16
    L, R = cases.textured_pair(9500 + 10 * cw + ch, W, H, 4, top=7, noise=1)
    kw = dict(numDisparities=D, blockSize=3, paths=5, speckleWindowSize=0)
    m = matcher(pkg, W, H, (cw, ch), **kw)
    try:
        assert_same(m.compute(L, R), ref.sgm_compute(L, R, census=(cw, ch), **kw), "%dx%d" % (cw, ch))
    finally:
        m.close()


# ---- 2. refusal --------------------------------------------------------------------------------------------------------------------
def test_refused_frame_then_a_good_one(pkg):
    W, H = 72, 24
    L, R = cases.noise_pair(9200, W, H)
    kw = dict(numDisparities=16, blockSize=5, P2=32000, paths=8)
    with pytest.raises(ref.CostOverflow):
        ref.sgm_compute(L, R, census=(9, 7), **kw)
    m = matcher(pkg, W, H, (9, 7), **kw)
    try:
        out = np.empty((H, W), np.int16)
        lib = pkg.binding.lib()
        assert lib.rtdm_sgm_compute(m._h, L.ctypes.data, W, R.ctypes.data, W, W, H, out.ctypes.data, W * 2) == -6
        flat = np.full((H, W), 90, np.uint8)
        assert lib.rtdm_sgm_compute(m._h, flat.ctypes.data, W, flat.ctypes.data, W, W, H, out.ctypes.data, W * 2) == 0
        assert_same(out, ref.sgm_compute(flat, flat, census=(9, 7), **kw), "constant pair after a refusal")
        # and through the device entry point, which reads the flag back itself
        rc, _ = device_call(pkg, m, L[None], R[None])
        assert rc == -6
        rc, got = device_call(pkg, m, flat[None], flat[None])
        assert rc == 0
        assert_same(got[0], out)
    finally:
        m.close()


# ---- 3. switching on one handle ------------------------------------------------------------------------------------------------------
def test_census_then_bt_on_one_handle(pkg, oracle):
    W, H = 110, 28
    L, R = cases.textured_pair(9400, W, H, 7)
    kw = dict(numDisparities=32, blockSize=5, paths=8)
    want_bt63 = sgm_cn_ref.sgm_compute_cn(L, R, preFilterCap=63, **kw)
    assert (want_bt63 != oracle.sgm_compute(L, R, **kw)).any()
    want_census = ref.sgm_compute(L, R, census=(7, 5), **kw)
    fresh = matcher(pkg, W, H, None, cap=63, **kw)
    try:
        fresh_bt = fresh.compute(L, R)
        assert fresh.getCost() == (fresh.COST_BT, (9, 7))
    finally:
        fresh.close()
    assert_same(fresh_bt, want_bt63, "fresh BT handle")
    m = matcher(pkg, W, H, None, **kw)
    lib = pkg.binding.lib()
    try:
        m.setPreFilterCap(63)                                                     # stored, without effect under census (N3)
        m.setCost(m.COST_CENSUS, (7, 5))
        assert_same(m.compute(L, R), want_census, "census")
        m.setPreFilterCap(0)
        assert_same(m.compute(L, R), want_census, "census at another preFilterCap")
        m.setPreFilterCap(63)
        # refused settings leave the handle as it is
        for bad in ((2, 9, 7), (-1, 9, 7), (1, 4, 7), (1, 9, 9), (1, 11, 3), (1, 0, 0), (1, 7, 1)):
            assert lib.rtdm_sgm_set_cost(m._h, *bad) == -1, bad
        assert m.getCost() == (m.COST_CENSUS, (7, 5))
        assert lib.rtdm_sgm_get_cost(m._h, None, None, None) == 0
        m.setCost(m.COST_BT, (4, 4))                                              # BT ignores the sizes
        assert m.getCost() == (m.COST_BT, (7, 5))
        got = m.compute(L, R)
        assert_same(got, want_bt63, "BT after census")
        assert got.tobytes() == fresh_bt.tobytes()
        m.setCost(m.COST_CENSUS)
        assert m.getCost() == (m.COST_CENSUS, (9, 7))
        assert_same(m.compute(L, R), ref.sgm_compute(L, R, census=(9, 7), **kw), "census again, 9 x 7")
    finally:
        m.close()


# ---- 4. invariance ---------------------------------------------------------------------------------------------------------------------
def test_increasing_mapping_of_one_view_changes_nothing_under_census(pkg):
    L, R, Rm = cases.lut_pair()
    H, W = L.shape
    kw = dict(numDisparities=32, blockSize=5, paths=5, speckleWindowSize=0)
    m = matcher(pkg, W, H, (9, 7), **kw)
    try:
        plain, mapped = m.compute(L, R), m.compute(L, Rm)
        assert plain.tobytes() == mapped.tobytes()
        assert_same(plain, ref.sgm_compute(L, R, census=(9, 7), **kw))
        assert (plain != -16).mean() > 0.3
        m.setCost(m.COST_BT)
        assert (m.compute(L, R) != m.compute(L, Rm)).any()                        # the BT cost does see the mapping
    finally:
        m.close()


# ---- 5. channel counts --------------------------------------------------------------------------------------------------------------------
def test_gray_only(pkg):
    import torch
    W, H = 80, 17
    L, R = cases.textured_pair(9600, W, H, 5)
    kw = dict(numDisparities=16, blockSize=5, paths=5)
    lib = pkg.binding.lib()
    m = matcher(pkg, W, H, (9, 7), **kw)
    try:
        out = np.empty((H, W), np.int16)
        assert lib.rtdm_sgm_compute_cn(m._h, 1, L.ctypes.data, W, R.ctypes.data, W, W, H, out.ctypes.data, W * 2) == 0
        assert_same(out, ref.sgm_compute(L, R, census=(9, 7), **kw))
        L3, R3 = np.repeat(L[:, :, None], 3, 2).copy(), np.repeat(R[:, :, None], 3, 2).copy()
        out3 = np.full((H, W), 77, np.int16)
        assert lib.rtdm_sgm_compute_cn(m._h, 3, L3.ctypes.data, W * 3, R3.ctypes.data, W * 3, W, H, out3.ctypes.data, W * 2) == -6
        assert (out3 == 77).all()
        with pytest.raises(pkg.binding.RtdmError) as e:
            m.compute(L3, R3)
        assert e.value.status == -6
        dL, dR = torch.from_numpy(L3[None]).cuda(), torch.from_numpy(R3[None]).cuda()
        dD = torch.full((1, H, W), 77, dtype=torch.int16, device="cuda")
        assert lib.rtdm_sgm_compute_device_cn(m._h, 3, 1, dL.data_ptr(), dR.data_ptr(), W * 3, W * H * 3, W, H, dD.data_ptr(), W * 2,
                                              W * H * 2, torch.cuda.current_stream().cuda_stream) == -6
        torch.cuda.synchronize()
        assert (dD == 77).all()
        # the argument checks the call makes today come first
        assert lib.rtdm_sgm_compute_cn(m._h, 2, L3.ctypes.data, W * 3, R3.ctypes.data, W * 3, W, H, out3.ctypes.data, W * 2) == -1
        assert lib.rtdm_sgm_compute_cn(m._h, 3, L3.ctypes.data, W, R3.ctypes.data, W * 3, W, H, out3.ctypes.data, W * 2) == -2
        # back on BT the handle takes colour
        m.setCost(m.COST_BT)
        assert_same(m.compute(L3, R3), sgm_cn_ref.sgm_compute_cn(L3, R3, **kw), "colour under BT")
    finally:
        m.close()


# ---- 6. the diagnostic switches ----------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def switch(pkg, name, value):
    getattr(pkg.binding.lib(), name)(value)
    try:
        yield
    finally:
        getattr(pkg.binding.lib(), name)(0)


@pytest.mark.parametrize("D,bs", [(32, 5), (48, 9)])
def test_debug_switches_do_not_change_a_byte(pkg, D, bs):
    W, H = D + 75, 23
    L, R = cases.textured_pair(9700 + D, W, H, 6)
    kw = dict(numDisparities=D, blockSize=bs, paths=8)
    want = ref.sgm_compute(L, R, census=(9, 7), **kw)

    def run():
        m = matcher(pkg, W, H, (9, 7), **kw)
        try:
            return m.compute(L, R), m.path_variant
        finally:
            m.close()
    plain, v0 = run()
    assert v0 in VARIANT[8]
    assert_same(plain, want)
    with switch(pkg, "rtdm_debug_sgm_cost16", 1):
        got, v = run()
    assert v == v0 and got.tobytes() == plain.tobytes()
    with switch(pkg, "rtdm_debug_sgm_wide_paths", 1):
        got, v = run()
    assert v == "wide_w1" and got.tobytes() == plain.tobytes()


# ---- 7. the right matcher -------------------------------------------------------------------------------------------------------------------
def test_right_matcher_carries_the_cost(pkg):
    W, H, D, minD = 150, 31, 32, 2
    L, R = cases.textured_pair(9800, W, H, 9)
    left = matcher(pkg, W, H, (7, 3), numDisparities=D, minDisparity=minD, blockSize=5, paths=5)
    right = pkg.create_right_matcher(left)
    try:
        assert right.getCost() == left.getCost() == (left.COST_CENSUS, (7, 3))
        p = right.params
        assert (p.minDisparity, p.uniquenessRatio, p.speckleWindowSize, p.paths) == (-(minD + D) + 1, 0, 0, 5)
        want = ref.sgm_compute(R, L, census=(7, 3), numDisparities=p.numDisparities, minDisparity=p.minDisparity,
                               blockSize=p.blockSize, P1=p.P1, P2=p.P2, uniquenessRatio=p.uniquenessRatio,
                               speckleWindowSize=p.speckleWindowSize, speckleRange=p.speckleRange, disp12MaxDiff=p.disp12MaxDiff,
                               paths=p.paths)
        assert_same(right.compute(R, L), want, "right")
        assert (want != (p.minDisparity - 1) * 16).mean() > 0.3
        assert_same(left.compute(L, R), ref.sgm_compute(L, R, census=(7, 3), numDisparities=D, minDisparity=minD, blockSize=5, paths=5))
    finally:
        right.close(); left.close()
    # a BT matcher's right matcher stays BT
    left = matcher(pkg, W, H, None, numDisparities=D, blockSize=5)
    right = pkg.create_right_matcher(left)
    try:
        assert right.getCost()[0] == right.COST_BT
    finally:
        right.close(); left.close()
