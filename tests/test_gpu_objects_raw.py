"""The object detection's own kernels on the masks an open + close never lets through (tests/cc_cases.py), and its HSV
conversion pixel by pixel, through the C ABI (rtdm_objects_detect).  Every detector here filters with ERODE by a 1x1 RECT,
the identity: the mask that detect() returns is k_hsv_inrange's own, and k_cc_rows / k_cc_merge / k_cc_bbox / k_cc_collect
label exactly the mask that was painted.  Everything is bit-exact against oracle/objects_oracle.c, which
tests/test_objects_cases_cpu.py holds against scipy and Python integers on the same inputs."""
import ctypes as C

import numpy as np
import pytest

import cc_cases as cc

pytestmark = pytest.mark.gpu

MAX_BOXES = 20000


@pytest.fixture(scope="module")
def pkg():
    import torch                         # torch first: it brings its own HIP runtime and must initialise before ours
    assert torch.cuda.is_available()
    from conftest import load
    return load()


def raw_detector(pkg, W, H):
    det = pkg.HIPObjectDetector(W, H)
    det.set_op(pkg.MORPH_ERODE, (pkg.MORPH_RECT, (1, 1)))
    return det


@pytest.fixture(scope="module")
def detectors(pkg):
    """One detector per frame size, kept for the whole module: every case of a size runs on the handle the case before it
    left behind, labels, boxes, count and record list included."""
    pool = {}

    def get(W, H):
        if (W, H) not in pool:
            pool[(W, H)] = raw_detector(pkg, W, H)
        return pool[(W, H)]

    yield get
    for det in pool.values():
        det.close()


def check_labelling(oracle, det, mask, min_area, zb, max_boxes=MAX_BOXES, rgb=None):
    boxes, roi, out = det.detect(cc.paint(mask) if rgb is None else rgb, min_area=min_area, zero_border=zb, max_boxes=max_boxes)
    assert np.array_equal(out, mask)                                           # the identity filter: the rest is the labelling's
    want = oracle.external_boxes(mask, min_area, zb, max_boxes=MAX_BOXES)
    assert len(want) < MAX_BOXES
    assert boxes == want[:max_boxes], (min_area, zb, len(boxes), len(want))
    assert roi == oracle.union_box(want)
    return want


@pytest.mark.parametrize("name", cc.NAMES)
def test_labelling(oracle, detectors, name):
    mask = cc.BY_NAME[name]
    det = detectors(mask.shape[1], mask.shape[0])
    for zb in (True, False):
        for min_area in (1, 12):
            check_labelling(oracle, det, mask, min_area, zb)


def test_more_records_than_the_first_download_holds_and_truncation(pkg, oracle):
    W, H = cc.BIG
    dots, rings = cc.BY_NAME["dots-%dx%d" % (W, H)], cc.BY_NAME["rings2-%dx%d" % (W, H)]
    det = raw_detector(pkg, W, H)
    for zb in (True, False):
        want = check_labelling(oracle, det, dots, 1, zb)
        assert len(want) == 8320
        check_labelling(oracle, det, dots, 1, zb, max_boxes=100)               # the first 100, the ROI of all 8320
        assert len(check_labelling(oracle, det, rings, 1, zb)) == 1            # nothing of the long list survives
        assert len(check_labelling(oracle, det, dots, 12, zb)) == 0
    det.close()


def test_rgb_rows_with_padding(oracle, detectors):
    mask = cc.BY_NAME["noise45-257x131/lr"]
    H, W = mask.shape
    buf = np.full((H, 3 * W + 7), 0x5a, np.uint8)
    rgb = np.lib.stride_tricks.as_strided(buf, (H, W, 3), (3 * W + 7, 3, 1))
    rgb[...] = cc.paint(mask)
    assert rgb.strides[0] == 3 * W + 7 and (buf[:, 3 * W:] == 0x5a).all()
    for zb in (True, False):
        check_labelling(oracle, detectors(W, H), mask, 1, zb, rgb=rgb)
    assert (buf[:, 3 * W:] == 0x5a).all()


def test_mask_rows_with_padding_through_the_raw_abi(pkg, oracle, detectors):
    B = pkg.binding
    mask = cc.BY_NAME["stairs-300x70"]
    H, W = mask.shape
    det = detectors(W, H)
    rgb = cc.paint(mask)
    out = np.full((H, W + 5), 0xa5, np.uint8)
    boxes = (B.Region * MAX_BOXES)(); n = C.c_int(); roi = B.Region()
    rng = B.HsvRange((C.c_int * 3)(*oracle.HSV_LOW), (C.c_int * 3)(*oracle.HSV_HIGH))
    B.check(B.lib().rtdm_objects_detect(det._h, rgb.ctypes.data, 3 * W, C.byref(rng), 1, 0, out.ctypes.data, W + 5, boxes, MAX_BOXES,
                                        C.byref(n), C.byref(roi)), "rtdm_objects_detect")
    assert np.array_equal(out[:, :W], mask) and (out[:, W:] == 0xa5).all()
    want = oracle.external_boxes(mask, 1, False, max_boxes=MAX_BOXES)
    assert [(b.x, b.y, b.width, b.height) for b in boxes[:n.value]] == want and len(want) > 50
    assert (roi.x, roi.y, roi.width, roi.height) == oracle.union_box(want)


def test_size_limits(pkg):
    det = pkg.HIPObjectDetector(8192, 4)
    det.close()
    with pytest.raises(pkg.binding.RtdmError):
        pkg.HIPObjectDetector(8193, 4)


# ---- HSV, exact per pixel ---------------------------------------------------------------------------------------------
NO_BOXES = 10 ** 9


def bands(det, rgb, channel, values, top=None):
    """Plane of `channel` rebuilt from single-value ranges: the value whose mask holds the pixel.  Asserts that every pixel
    lies in exactly one band.  top: one more range [top, 255], which has to be empty."""
    H, W, _ = rgb.shape
    plane = np.zeros((H, W), np.int32)
    seen = np.zeros((H, W), np.int32)
    for t in values:
        lo, hi = [0, 0, 0], [255, 255, 255]
        lo[channel] = hi[channel] = t
        boxes, _, m = det.detect(rgb, low=lo, high=hi, min_area=NO_BOXES, zero_border=False)
        assert boxes == [] and set(np.unique(m).tolist()) <= {0, 255}
        plane[m != 0] = t
        seen += m != 0
    assert (seen == 1).all(), (channel, np.unique(seen).tolist())
    if top is not None:
        lo, hi = [0, 0, 0], [255, 255, 255]
        lo[channel] = top
        assert not det.detect(rgb, low=lo, high=hi, min_area=NO_BOXES, zero_border=False)[2].any()
    return plane


@pytest.fixture(scope="module")
def hsv_frame(oracle):
    rgb = cc.hsv_frame()
    return rgb, oracle.rgb2hsv(rgb)


@pytest.fixture(scope="module")
def sat_frame(oracle):
    rgb = cc.sat_frame()
    return rgb, oracle.rgb2hsv(rgb)


def test_hue_of_every_pixel(detectors, hsv_frame):
    rgb, want = hsv_frame
    got = bands(detectors(rgb.shape[1], rgb.shape[0]), rgb, 0, range(180), top=180)
    assert np.array_equal(got, want[..., 0])


def test_saturation_of_every_pixel(detectors, sat_frame):
    rgb, want = sat_frame
    got = bands(detectors(rgb.shape[1], rgb.shape[0]), rgb, 1, range(256))
    assert np.array_equal(got, want[..., 1])


def test_value_of_every_pixel(detectors, sat_frame):
    rgb, want = sat_frame
    got = bands(detectors(rgb.shape[1], rgb.shape[0]), rgb, 2, range(256))
    assert np.array_equal(got, want[..., 2])


def test_saturation_and_value_of_the_hue_block(detectors, hsv_frame):
    # the whole frame in 16 coarse bands per channel: s and v of the pixels the two tests above do not see
    rgb, want = hsv_frame
    det = detectors(rgb.shape[1], rgb.shape[0])
    for ch in (1, 2):
        for t in range(0, 256, 16):
            lo, hi = [0, 0, 0], [255, 255, 255]
            lo[ch], hi[ch] = t, t + 15
            m = det.detect(rgb, low=lo, high=hi, min_area=NO_BOXES, zero_border=False)[2]
            assert np.array_equal(m != 0, (want[..., ch] >= t) & (want[..., ch] <= t + 15)), (ch, t)


def test_random_ranges(oracle, detectors, hsv_frame):
    rgb, _ = hsv_frame
    det = detectors(rgb.shape[1], rgb.shape[0])
    for i, (lo, hi) in enumerate(cc.random_ranges()):
        m = det.detect(rgb, low=lo, high=hi, min_area=NO_BOXES, zero_border=False)[2]
        assert np.array_equal(m, oracle.hsv_inrange(rgb, lo, hi)), (i, lo, hi)
        if i == 1:
            assert not m.any()                                                 # low > high in a channel
