"""StereoSGBM with colour frames and preFilterCap (rtdm_sgm_compute_cn, rtdm_sgm_compute_device_cn,
rtdm_sgm_set_prefilter_cap): every result is compared bit for bit with sgm_cn_ref.sgm_compute_cn (the NumPy restatement of R1
chained through the C oracle's later stages).  rtdm_debug_sgm_cost16 forces the 16-bit pixel-cost forms on gray frames, so
that they can be held against the shipped 8-bit forms; it is reset in `finally` everywhere."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import sgm_cn_ref as ref
from conftest import load

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    import torch                         # torch first: it brings its own HIP runtime and must initialise before ours
    assert torch.cuda.is_available(), "the -m gpu suite needs an MI355X"
    return load()


@contextlib.contextmanager
def forced_cost16(pkg):
    pkg.binding.lib().rtdm_debug_sgm_cost16(1)
    try:
        yield
    finally:
        pkg.binding.lib().rtdm_debug_sgm_cost16(0)


def assert_same(got, want, what=""):
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError("%s: %d / %d pixels differ; first at (y,x)=%s got %d want %d" % (
            what, len(bad), got.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])]))


def pair(seed, W, H, shift, cn):
    """A textured pair whose right view is the left one moved by `shift` columns, gray (H x W) or colour (H x W x 3)."""
    rng = np.random.default_rng(seed)
    T = rng.integers(0, 256, (H, W + abs(shift), cn)).astype(np.float64)
    T = (T + np.roll(T, 1, 1) + np.roll(T, -1, 1) + np.roll(T, 1, 0) + np.roll(T, -1, 0)) / 5
    T = T.astype(np.uint8)
    if shift >= 0:
        L, R = T[:, :W], T[:, shift:shift + W]
    else:
        L, R = T[:, -shift:-shift + W], T[:, :W]
    L, R = L.copy(), R.copy()
    return (L[:, :, 0].copy(), R[:, :, 0].copy()) if cn == 1 else (L, R)


def run(pkg, L, R, cap, max_batch=1, **kw):
    H, W = L.shape[:2]
    kw = dict(kw)
    kw["numOfDisparities"] = kw.pop("numDisparities")
    m = pkg.HIPSemiGlobalMatcher(width=W, height=H, max_batch=max_batch, preFilterCap=cap, **kw)
    try:
        return m.compute(L, R)
    finally:
        m.close()


# ---- 1. colour and gray across caps, modes, numDisparities, windows and minDisparity ------------------------------------------
CASES = [
    # cn, cap, paths, D, blockSize, minD, W, H
    (3, 0, 5, 16, 5, 0, 97, 31),
    (3, 16, 8, 64, 3, -7, 181, 40),
    (3, 31, 5, 128, 1, 5, 263, 28),
    (3, 63, 8, 256, 7, 0, 331, 20),
    (3, 96, 5, 64, 9, -20, 161, 33),
    (3, 97, 8, 16, 11, 3, 77, 37),
    (3, 127, 5, 272, 3, 0, 353, 18),
    (3, 63, 8, 512, 5, -9, 581, 12),
    (3, 15, 8, 128, 9, -64, 221, 24),
    (3, 0, 5, 32, 7, 0, 121, 26),
    (1, 16, 8, 64, 5, 0, 151, 29),
    (1, 31, 5, 128, 3, -3, 241, 25),
    (1, 63, 8, 256, 7, 2, 319, 21),
    (1, 96, 5, 16, 9, 0, 67, 35),
    (1, 97, 8, 64, 5, -11, 143, 30),
    (1, 127, 5, 128, 1, 0, 203, 27),
    (1, 127, 8, 272, 11, 0, 345, 16),
    (1, 97, 5, 512, 3, 4, 557, 10),
    (1, 63, 8, 128, 9, 0, 209, 30),
]


@pytest.mark.parametrize("cn,cap,paths,D,bs,minD,W,H", CASES)
def test_bit_exact(pkg, cn, cap, paths, D, bs, minD, W, H):
    L, R = pair(9000 + D + cap + bs + cn, W, H, minD + min(D - 1, 13), cn)
    kw = dict(numDisparities=D, blockSize=bs, minDisparity=minD, paths=paths)
    want = ref.sgm_compute_cn(L, R, preFilterCap=cap, **kw)
    got = run(pkg, L, R, cap, **kw)
    assert_same(got, want, "cn=%d cap=%d paths=%d D=%d bs=%d minD=%d" % (cn, cap, paths, D, bs, minD))
    assert (want != (minD - 1) * 16).mean() > 0.05


# ---- 2. the device entry point: batches, including more frames than max_batch -----------------------------------------------
@pytest.mark.parametrize("cn,cap,n,max_batch", [(3, 63, 3, 4), (3, 0, 5, 2), (1, 127, 4, 3)])
def test_device_batches(pkg, cn, cap, n, max_batch):
    import torch
    W, H, D = 150, 26, 64
    frames = [pair(9500 + i + cap, W, H, 4 + 3 * i, cn) for i in range(n)]
    Ls = np.stack([f[0] for f in frames]); Rs = np.stack([f[1] for f in frames])
    kw = dict(numDisparities=D, blockSize=5, paths=5)
    m = pkg.HIPSemiGlobalMatcher(numOfDisparities=D, blockSize=5, paths=5, width=W, height=H, max_batch=max_batch,
                                 preFilterCap=cap)
    try:
        dL, dR = torch.from_numpy(Ls).cuda(), torch.from_numpy(Rs).cuda()
        dD = torch.empty((n, H, W), dtype=torch.int16, device="cuda")
        m.compute_device(dL, dR, dD, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        got = dD.cpu().numpy()
    finally:
        m.close()
    for i in range(n):
        assert_same(got[i], ref.sgm_compute_cn(Ls[i], Rs[i], preFilterCap=cap, **kw), "frame %d" % i)


# ---- 3. channels = 1 through the _cn entry points is the old entry point --------------------------------------------------------
def test_channels_one_is_rtdm_sgm_compute(pkg, synth):
    B = pkg.binding
    lib = B.lib()
    W, H, D = 203, 47, 64
    L, R = synth.make_pair(synth.STREAM_SEED + 9600, W, H, D)
    p = B.SGMParams(5, 0, D, 600, 2400, 10, 100, 32, 1, 5)
    h = C.c_void_p()
    B.check(lib.rtdm_sgm_create(C.byref(p), W, H, 1, 0, C.byref(h)), "rtdm_sgm_create")
    try:
        a = np.empty((H, W), np.int16); b = np.empty((H, W), np.int16)
        B.check(lib.rtdm_sgm_compute(h, L.ctypes.data, W, R.ctypes.data, W, W, H, a.ctypes.data, W * 2), "rtdm_sgm_compute")
        B.check(lib.rtdm_sgm_compute_cn(h, 1, L.ctypes.data, W, R.ctypes.data, W, W, H, b.ctypes.data, W * 2),
                "rtdm_sgm_compute_cn")
    finally:
        lib.rtdm_sgm_destroy(h)
    assert a.tobytes() == b.tobytes()
    assert_same(a, ref.sgm_compute_cn(L, R, numDisparities=D, blockSize=5, paths=5))


@pytest.mark.parametrize("cn", [1, 3])
def test_pitched_views_and_odd_width(pkg, cn):
    W, H, D, cap = 133, 23, 32, 31
    L, R = pair(9700 + cn, W + 9, H, 5, cn)
    Lv, Rv = L[:, 4:4 + W], R[:, 2:2 + W]            # row pitch (W + 9) * cn bytes
    assert Lv.strides[0] == (W + 9) * cn
    kw = dict(numDisparities=D, blockSize=3, paths=8)
    assert_same(run(pkg, Lv, Rv, cap, **kw), ref.sgm_compute_cn(Lv, Rv, preFilterCap=cap, **kw))


# ---- 4. the 16-bit pixel-cost forms against the 8-bit ones on gray frames -----------------------------------------------------
@pytest.mark.parametrize("D,bs,cap,paths", [(16, 1, 0, 5), (64, 3, 0, 8), (128, 5, 15, 5), (256, 7, 63, 8), (64, 9, 0, 5),
                                            (128, 13, 31, 8), (32, 19, 0, 5), (512, 5, 0, 8), (96, 7, 0, 5)])
def test_cost16_forms_equal_u8_forms(pkg, D, bs, cap, paths):
    W, H = D + 97, 33
    L, R = pair(9800 + D + bs, W, H, min(D - 1, 11), 1)
    kw = dict(numDisparities=D, blockSize=bs, paths=paths)
    u8 = run(pkg, L, R, cap, **kw)
    with forced_cost16(pkg):
        u16 = run(pkg, L, R, cap, **kw)
    assert u8.tobytes() == u16.tobytes()
    assert_same(u8, ref.sgm_compute_cn(L, R, preFilterCap=cap, **kw))


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bs,P2,cap", [(17, 2400, 63), (7, 30000, 127), (31, 2400, 0)])
def test_overflowing_colour_frame_is_refused(pkg, bs, P2, cap):
    """unrelated binary noise in the two views: block costs + P2 pass 32767 -- the frame is refused, never wrapped; the handle
    then serves a frame that fits"""
    rng = np.random.default_rng(bs)
    W, H, D = 120, 40, 16
    L, R = (rng.integers(0, 2, (2, H, W, 3)) * 255).astype(np.uint8)
    kw = dict(numDisparities=D, blockSize=bs, P2=P2, speckleWindowSize=0)
    with pytest.raises(ref.CostOverflow):
        ref.sgm_compute_cn(L, R, preFilterCap=cap, **kw)
    m = pkg.HIPSemiGlobalMatcher(numOfDisparities=D, blockSize=bs, P2=P2, speckleWindowSize=0, width=W, height=H,
                                 preFilterCap=cap)
    try:
        with pytest.raises(pkg.binding.RtdmError) as e:
            m.compute(L, R)
        assert e.value.status == -6
        Lf, Rf = pair(9900 + bs, W, H, 3, 3)
        Lf = (Lf // 32).astype(np.uint8); Rf = (Rf // 32).astype(np.uint8)   # low contrast: small costs
        want = ref.sgm_compute_cn(Lf, Rf, preFilterCap=cap, **kw)
        assert_same(m.compute(Lf, Rf), want, "after a refused frame")
    finally:
        m.close()


def test_refusals(pkg):
    B = pkg.binding
    lib = B.lib()
    W, H = 64, 16
    with pytest.raises(B.RtdmError) as e:
        pkg.HIPSemiGlobalMatcher(numOfDisparities=16, width=W, height=H, preFilterCap=128)
    assert e.value.status == -6
    m = pkg.HIPSemiGlobalMatcher(numOfDisparities=16, width=W, height=H)
    try:
        assert lib.rtdm_sgm_set_prefilter_cap(m._h, 128) == -6
        assert lib.rtdm_sgm_set_prefilter_cap(m._h, 200) == -6
        assert lib.rtdm_sgm_set_prefilter_cap(m._h, 127) == 0
        buf = np.zeros((H, W, 4), np.uint8); out = np.empty((H, W), np.int16)
        for cn in (0, 2, 4):
            assert lib.rtdm_sgm_compute_cn(m._h, cn, buf.ctypes.data, W * 4, buf.ctypes.data, W * 4, W, H,
                                           out.ctypes.data, W * 2) == -1
            assert lib.rtdm_sgm_compute_device_cn(m._h, cn, 1, buf.ctypes.data, buf.ctypes.data, W * 4, W * H * 4, W, H,
                                                  out.ctypes.data, W * 2, W * H * 2, None) == -1
        # a row holds channels * width bytes
        assert lib.rtdm_sgm_compute_cn(m._h, 3, buf.ctypes.data, W * 2, buf.ctypes.data, W * 3, W, H, out.ctypes.data,
                                       W * 2) == -2
        with pytest.raises(ValueError):
            m.compute(buf[:, :, :2].copy(), buf[:, :, :2].copy())
        with pytest.raises(TypeError):
            m.compute(buf[:, :, 0].astype(np.uint16), buf[:, :, 0].astype(np.uint16))
        with pytest.raises(ValueError):
            m.compute(buf[:, :, :3].copy(), buf[:, :, 0].copy())
    finally:
        m.close()


# ---- 6. the Python API end to end: setPreFilterCap applies from the next call ---------------------------------------------------
def test_python_api_end_to_end(pkg):
    W, H, D = 220, 36, 64
    L3, R3 = pair(9990, W, H, 9, 3)
    m = pkg.HIPSemiGlobalMatcher(numOfDisparities=D, blockSize=3, width=W, height=H, paths=5)
    try:
        kw = dict(numDisparities=D, blockSize=3, paths=5)
        assert_same(m.compute(L3, R3), ref.sgm_compute_cn(L3, R3, preFilterCap=0, **kw), "colour, cap 0")
        m.setPreFilterCap(63)
        assert m.preFilterCap == 63
        got63 = m.compute(L3, R3)
        assert_same(got63, ref.sgm_compute_cn(L3, R3, preFilterCap=63, **kw), "colour, cap 63")
        g = np.ascontiguousarray(L3[:, :, 1]); h = np.ascontiguousarray(R3[:, :, 1])
        assert_same(m.compute(g, h), ref.sgm_compute_cn(g, h, preFilterCap=63, **kw), "gray after colour, cap 63")
    finally:
        m.close()
