"""The batched, multi-class object detection on the device (rtdm_objects_detect_device, rtdm_objects_detect_batch,
rtdm_estimate_frame_classes; rules O1-O6 of DESIGN.md section 4.15) against tests/objects_batch_ref.py, which is built from the
oracle's single-mask pieces.  Unless a test says otherwise the detector filters with ERODE by a 1x1 RECT (the identity), so
that the planes that are labelled are the planes that were painted: class 0 = red OR green pixels, class 1 = blue OR green
(objects_batch_ref.paint2).  Masks, objects, counts and union boxes are compared exactly; only the mean depth of the chain is a
floating-point sum in another order (1e-9 relative, the bound rtdm_bm_compute_depth is held to)."""
import ctypes as C

import numpy as np
import pytest

import cc_cases as cc
import objects_batch_ref as ref
import rectify_util as ru

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
NULL, BAD_PARAM, BAD_SIZE = -7, -1, -2


@pytest.fixture(scope="module")
def pkg():
    import torch                         # torch first: it brings its own HIP runtime and must initialise before ours
    assert torch.cuda.is_available()
    from conftest import load
    return load()


def raw_detector(pkg, W, H, max_batch=1, max_classes=1):
    det = pkg.HIPObjectDetector(W, H, max_batch=max_batch, max_classes=max_classes)
    det.set_op(pkg.MORPH_ERODE, (pkg.MORPH_RECT, (1, 1)))
    return det


def prepare(rgbs, classes=ref.TWO_CLASSES, capacity=20000):
    """Contiguous torch tensors of one rtdm_objects_detect_device call: the frames, and outputs that start as SENTINEL bytes.
    Enqueued on torch's current stream and NOT synchronised."""
    import torch
    n, H, W, _ = rgbs.shape
    K = max(classes) + 1
    return dict(rgb=torch.from_numpy(np.ascontiguousarray(rgbs)).cuda(),
                objects=torch.full((n, capacity * 32), SENTINEL, dtype=torch.uint8, device="cuda"),
                counts=torch.full((n, K), -7, dtype=torch.int32, device="cuda"),
                rois=torch.full((n, 4), -7, dtype=torch.int32, device="cuda"),
                masks=torch.full((n, K, H, W), SENTINEL, dtype=torch.uint8, device="cuda"), capacity=capacity)


def issue(det, t, ranges=ref.TWO_RANGES, classes=ref.TWO_CLASSES, min_area=1, zero_border=True, stream=None):
    """The call itself on `stream`, nothing before it and nothing behind it."""
    det.detect_device(t["rgb"], ranges, classes, t["objects"], t["counts"], t["rois"], d_masks=t["masks"], min_area=min_area,
                      zero_border=zero_border, capacity=t["capacity"], stream=stream)


def run_device(pkg, det, rgbs, ranges=ref.TWO_RANGES, classes=ref.TWO_CLASSES, capacity=20000, min_area=1, zero_border=True):
    """prepare, one device synchronisation, issue on the null stream, host() -> dict(objects n x capacity OBJECT_DTYPE,
    counts n x K, rois n x 4, masks n x K x H x W)."""
    import torch
    t = prepare(rgbs, classes, capacity)
    torch.cuda.synchronize()
    issue(det, t, ranges, classes, min_area, zero_border)
    return host(t)


def host(out):
    import torch
    torch.cuda.synchronize()
    n = out["objects"].shape[0]
    return dict(objects=out["objects"].cpu().numpy().view(np.dtype(OBJECT)).reshape(n, -1), counts=out["counts"].cpu().numpy(),
                rois=out["rois"].cpu().numpy(), masks=out["masks"].cpu().numpy())


OBJECT = [(n, "<i4") for n in ("x", "y", "width", "height", "cls", "first_pixel")] + [("reserved", "<i4", (2,))]


def check_frame(got, f, want, capacity, W):
    """Frame f of a device result against objects_batch_ref.detect's dict: O1-O4 and what first_pixel and reserved must hold."""
    K = len(want["counts"])
    for c in range(K):
        assert np.array_equal(got["masks"][f, c], want["masks"][c]), ("mask", f, c)
    assert got["counts"][f].tolist() == want["counts"], (f, got["counts"][f].tolist(), want["counts"])
    assert tuple(got["rois"][f].tolist()) == want["roi"], (f, got["rois"][f].tolist(), want["roi"])
    stored = min(len(want["objects"]), capacity)
    o = got["objects"][f]
    have = list(zip(o["x"][:stored].tolist(), o["y"][:stored].tolist(), o["width"][:stored].tolist(), o["height"][:stored].tolist(),
                    o["cls"][:stored].tolist()))
    assert have == want["objects"][:stored], (f, stored)
    assert o[stored:].tobytes() == bytes([SENTINEL]) * (32 * (len(o) - stored)), "entries past the stored ones were written"
    assert not o["reserved"][:stored].any()
    # first_pixel: on the box's first row, inside the box, a foreground pixel of its class, descending inside a class
    fp, ys, xs = o["first_pixel"][:stored], o["first_pixel"][:stored] // W, o["first_pixel"][:stored] % W
    assert (ys == o["y"][:stored]).all() and (xs >= o["x"][:stored]).all() and (xs < o["x"][:stored] + o["width"][:stored]).all()
    for c in range(K):
        sel = o["cls"][:stored] == c
        assert (want["masks"][c][ys[sel], xs[sel]] != 0).all()
        assert (np.diff(fp[sel]) < 0).all()


def six_planes(W, H):
    m = cc.noise(W, H, 0.45, 7 * W + H)
    return [m, np.ascontiguousarray(m[:, ::-1]), np.ascontiguousarray(m[::-1]), np.roll(m, 5, 1), np.roll(m, 3, 0), np.roll(m[:, ::-1], 7, 1)]


@pytest.mark.parametrize("W,H", [(257, 131), (255, 131), (256, 131)])
def test_plane_indexing(pkg, oracle, W, H):
    planes = six_planes(W, H)
    assert all(not np.array_equal(a, b) for i, a in enumerate(planes) for b in planes[:i])
    rgbs = np.stack([ref.paint2(planes[2 * f], planes[2 * f + 1]) for f in range(3)])
    det = raw_detector(pkg, W, H, max_batch=4, max_classes=2)
    one = raw_detector(pkg, W, H)
    for zb in (True, False):
        got = run_device(pkg, det, rgbs, min_area=1, zero_border=zb)
        for f in range(3):
            check_frame(got, f, ref.detect(oracle, rgbs[f], ref.TWO_RANGES, ref.TWO_CLASSES, 1, zb), 20000, W)
            for c in range(2):                   # ... and against the single-frame detector on that plane alone
                boxes, _, out = one.detect(cc.paint(planes[2 * f + c]), min_area=1, zero_border=zb, max_boxes=20000)
                o = got["objects"][f][:got["counts"][f].sum()]
                o = o[o["cls"] == c]
                assert np.array_equal(out, got["masks"][f, c])
                assert boxes == list(zip(o["x"].tolist(), o["y"].tolist(), o["width"].tolist(), o["height"].tolist()))
    det.close(); one.close()


def test_plane_indexing_on_the_widest_frame(pkg, oracle):
    W, H = 8192, 4
    a, b = cc.runs(W, H, 1, 700), cc.runs(W, H, 2, 90)
    rgbs = ref.paint2(a, b)[None]
    det = raw_detector(pkg, W, H, max_classes=2)
    for zb in (True, False):
        got = run_device(pkg, det, rgbs, zero_border=zb)
        check_frame(got, 0, ref.detect(oracle, rgbs[0], ref.TWO_RANGES, ref.TWO_CLASSES, 1, zb), 20000, W)
    det.close()


@pytest.fixture(scope="module")
def five_frames():
    W, H = cc.BIG
    names = ["noise45", "rings_cut2", "border", "stairs", "noise60", "spiral", "comb", "quiet", "checker", "rings_cut_outer2"]
    planes = [np.zeros((H, W), np.uint8) if n == "quiet" else cc.BY_NAME["%s-%dx%d" % (n, W, H)] for n in names]
    return np.stack([ref.paint2(planes[2 * f], planes[2 * f + 1]) for f in range(5)])


def test_chunking(pkg, oracle, five_frames):
    W, H = cc.BIG
    results = []
    for mb in (2, 8):
        det = raw_detector(pkg, W, H, max_batch=mb, max_classes=2)
        results.append(run_device(pkg, det, five_frames, capacity=3000))
        det.close()
    det = raw_detector(pkg, W, H, max_classes=2)
    singles = [run_device(pkg, det, five_frames[f:f + 1], capacity=3000) for f in range(5)]
    results.append({k: np.concatenate([s[k] for s in singles]) for k in singles[0]})
    det.close()
    for f in range(5):
        check_frame(results[0], f, ref.detect(oracle, five_frames[f], ref.TWO_RANGES, ref.TWO_CLASSES, 1, True), 3000, W)
    for r in results[1:]:
        for k in r:
            assert r[k].tobytes() == results[0][k].tobytes(), k


def test_order_and_truncation(pkg, oracle):
    W, H = cc.BIG
    dots, rings = cc.BY_NAME["dots-%dx%d" % (W, H)], cc.BY_NAME["rings2-%dx%d" % (W, H)]
    rgbs = ref.paint2(dots, rings)[None]
    det = raw_detector(pkg, W, H, max_classes=2)
    want = ref.detect(oracle, rgbs[0], ref.TWO_RANGES, ref.TWO_CLASSES, 1, True)
    assert want["counts"] == [8320, 1]
    for capacity in (20000, 100, 8321, 8320, 0):        # whole; cut inside class 0; class 1's entry is the last; cut before it; nothing
        got = run_device(pkg, det, rgbs, capacity=capacity)
        check_frame(got, 0, want, capacity, W)          # counts and the union box are those of all 8321 whatever the capacity
    want = ref.detect(oracle, rgbs[0], ref.TWO_RANGES, ref.TWO_CLASSES, 12, True)
    assert want["counts"] == [0, 1]
    check_frame(run_device(pkg, det, rgbs, min_area=12, capacity=100), 0, want, 100, W)
    det.close()


def test_an_empty_frame_between_two_others(pkg, oracle, five_frames):
    W, H = cc.BIG
    rgbs = np.stack([five_frames[0], np.full((H, W, 3), 128, np.uint8), five_frames[2]])
    det = raw_detector(pkg, W, H, max_batch=3, max_classes=2)
    got = run_device(pkg, det, rgbs, capacity=3000)
    for f in range(3):
        check_frame(got, f, ref.detect(oracle, rgbs[f], ref.TWO_RANGES, ref.TWO_CLASSES, 1, True), 3000, W)
    assert got["counts"][1].tolist() == [0, 0] and tuple(got["rois"][1].tolist()) == oracle.union_box([])
    assert got["counts"][0].sum() > 0 and got["counts"][2].sum() > 0
    # ... which is what rtdm_objects_detect says of an empty frame
    boxes, roi, _ = det.detect(rgbs[1], min_area=1)
    assert boxes == [] and roi == tuple(got["rois"][1].tolist())
    det.close()


def test_or_of_ranges(pkg, oracle):
    rgb = cc.hsv_frame()
    H, W, _ = rgb.shape
    ranges = [((0, 100, 50), (9, 255, 255)), ((170, 100, 50), (179, 255, 255))] + cc.random_ranges(10)[2:]
    classes = [0, 0, 1, 2, 1, 2, 1, 2, 1, 2]
    assert len(ranges) == 10
    det = raw_detector(pkg, W, H, max_classes=3)
    got = run_device(pkg, det, rgb[None], ranges, classes, capacity=20000, min_area=20, zero_border=False)
    want = ref.detect(oracle, rgb, ranges, classes, 20, False)
    assert all(m.any() for m in want["masks"]) and len(want["objects"]) < 20000
    check_frame(got, 0, want, 20000, W)
    hue = oracle.rgb2hsv(rgb)[..., 0]
    assert (got["masks"][0, 0][hue >= 170] != 0).any() and (got["masks"][0, 0][hue <= 9] != 0).any()
    # the host entry point with the same classes
    objs, rois, counts, masks = det.detect_classes(rgb[None], ranges, classes, min_area=20, zero_border=False, capacity=20000)
    assert objs[0] == want["objects"] and rois[0] == want["roi"] and counts[0].tolist() == want["counts"]
    assert all(np.array_equal(masks[0, c], want["masks"][c]) for c in range(3))
    det.close()


@pytest.mark.parametrize("channel", [0, 1, 2])
def test_every_pixel_through_sixteen_ranges_in_eight_classes(pkg, oracle, channel):
    """The conversion per pixel, at the limits of a call: sixteen single-value ranges of one channel, two per class, per call;
    the class planes of all calls together say the channel's value of every pixel (hue on cc.hsv_frame, saturation and value
    on cc.sat_frame, as tests/test_gpu_objects_raw.py does with one range per call)."""
    rgb = cc.hsv_frame() if channel == 0 else cc.sat_frame()
    want = oracle.rgb2hsv(rgb)[..., channel].astype(np.int32)
    H, W, _ = rgb.shape
    det = raw_detector(pkg, W, H, max_classes=8)
    seen = np.zeros((H, W), np.int32)
    classes = [i % 8 for i in range(16)]
    for t0 in range(0, 256, 16):
        ranges = []
        for t in range(t0, t0 + 16):
            lo, hi = [0, 0, 0], [255, 255, 255]
            lo[channel] = hi[channel] = t
            ranges.append((lo, hi))
        _, _, counts, masks = det.detect_classes(rgb[None], ranges, classes, min_area=10 ** 9, zero_border=False, capacity=0)
        assert not counts.any() and set(np.unique(masks).tolist()) <= {0, 255}
        for c in range(8):
            hit = masks[0, c] != 0
            assert np.array_equal(hit, (want == t0 + c) | (want == t0 + c + 8)), (channel, t0, c)
            seen += hit
    assert (seen == 1).all()                              # every pixel in exactly one of the 256 bands
    det.close()


def blobs(W, H, seed, q):
    from scipy import ndimage as ndi
    rng = np.random.default_rng(seed)
    field = ndi.uniform_filter(rng.random((H, W)), 15)
    return ((field > np.quantile(field, q)) * 255).astype(np.uint8)


def test_a_real_filter(pkg, oracle):
    W, H = 233, 156                                      # the reference's crop at 320 x 240
    rgbs = np.stack([ref.paint2(blobs(W, H, 50 + f, 0.6), blobs(W, H, 60 + f, 0.75)) for f in range(2)])
    det = pkg.HIPObjectDetector(W, H, max_batch=2, max_classes=2)          # the default open + close
    for zb, area in ((True, 100), (False, 1)):
        got = run_device(pkg, det, rgbs, capacity=512, min_area=area, zero_border=zb)
        for f in range(2):
            want = ref.detect(oracle, rgbs[f], ref.TWO_RANGES, ref.TWO_CLASSES, area, zb, oracle.morph_open_close)
            assert all(want["counts"])
            check_frame(got, f, want, 512, W)
    det.close()


def test_pitches(pkg, oracle, five_frames):
    import torch
    W, H = cc.BIG
    n, K, cap = 3, 2, 3000
    pitch, fstride = 3 * W + 7, (3 * W + 7) * H + 13
    buf = torch.full((n * fstride,), 0x5a, dtype=torch.uint8, device="cuda")
    d_rgb = torch.as_strided(buf, (n, H, W, 3), (fstride, pitch, 3, 1))
    d_rgb.copy_(torch.from_numpy(five_frames[:n]).cuda())
    mbuf = torch.full((n, K, H + 1, W + 5), SENTINEL, dtype=torch.uint8, device="cuda")
    d_msk = mbuf[:, :, :H, :W]
    d_obj = torch.full((n, cap * 32), SENTINEL, dtype=torch.uint8, device="cuda")
    d_cnt = torch.zeros((n, K), dtype=torch.int32, device="cuda"); d_roi = torch.zeros((n, 4), dtype=torch.int32, device="cuda")
    det = raw_detector(pkg, W, H, max_batch=2, max_classes=2)
    det.detect_device(d_rgb, ref.TWO_RANGES, ref.TWO_CLASSES, d_obj, d_cnt, d_roi, d_masks=d_msk, min_area=1)
    got = host(dict(objects=d_obj, counts=d_cnt, rois=d_roi, masks=d_msk.contiguous()))
    for f in range(n):
        check_frame(got, f, ref.detect(oracle, five_frames[f], ref.TWO_RANGES, ref.TWO_CLASSES, 1, True), cap, W)
    m = mbuf.cpu().numpy()
    assert (m[:, :, :, W:] == SENTINEL).all() and (m[:, :, H:, :] == SENTINEL).all()          # the padding of the mask planes
    # the host entry point with padded rows and frames
    hb = np.full((n, H, 3 * W + 7), 0x5a, np.uint8)
    hrgb = np.lib.stride_tricks.as_strided(hb, (n, H, W, 3), (hb.strides[0], hb.strides[1], 3, 1))
    hrgb[...] = five_frames[:n]
    objs, rois, counts, masks = det.detect_classes(hrgb, ref.TWO_RANGES, ref.TWO_CLASSES, min_area=1, capacity=cap)
    for f in range(n):
        want = ref.detect(oracle, five_frames[f], ref.TWO_RANGES, ref.TWO_CLASSES, 1, True)
        assert objs[f] == want["objects"][:cap] and rois[f] == want["roi"] and counts[f].tolist() == want["counts"]
        assert all(np.array_equal(masks[f, c], want["masks"][c]) for c in range(K))
    det.close()


def test_two_calls_back_to_back_on_one_stream(pkg, oracle, five_frames):
    """Both calls' inputs and sentinel outputs are on the device first; then the two calls are enqueued on one stream with
    nothing between them -- no synchronisation, no other work -- on a handle whose max_batch makes each of them two chunks,
    so that four chunks share the handle's work planes in the queue.  One synchronisation, then both results are read."""
    import torch
    W, H = cc.BIG
    det = raw_detector(pkg, W, H, max_batch=2, max_classes=2)
    ta, tb = prepare(five_frames[0:3], capacity=3000), prepare(five_frames[2:5], capacity=3000)
    torch.cuda.synchronize()                             # the fills above ran on torch's stream: ordered before s once
    s = torch.cuda.Stream()
    issue(det, ta, stream=s.cuda_stream)
    issue(det, tb, zero_border=False, stream=s.cuda_stream)
    s.synchronize()
    a, b = host(ta), host(tb)
    for f in range(3):
        check_frame(a, f, ref.detect(oracle, five_frames[f], ref.TWO_RANGES, ref.TWO_CLASSES, 1, True), 3000, W)
        check_frame(b, f, ref.detect(oracle, five_frames[2 + f], ref.TWO_RANGES, ref.TWO_CLASSES, 1, False), 3000, W)
    det.close()


def test_run_to_run(pkg, five_frames):
    W, H = cc.BIG
    det = raw_detector(pkg, W, H, max_batch=3, max_classes=2)
    a = run_device(pkg, det, five_frames, capacity=3000)
    b = run_device(pkg, det, five_frames, capacity=3000)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    det.close()


def test_refusals_that_need_the_handle(pkg):
    import torch
    B = pkg.binding
    L = B.lib()
    W, H = 40, 12
    det = raw_detector(pkg, W, H, max_batch=2, max_classes=2)
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda").data_ptr()
    rng = (B.HsvRange * 3)(*[B.HsvRange((C.c_int * 3)(0, 0, 0), (C.c_int * 3)(255, 255, 255)) for _ in range(3)])

    def call(n=2, pitch=3 * W, fstride=3 * W * H, cls=(0, 1), nr=2, K=2, masks=buf, mpitch=W, mplane=W * H):
        return L.rtdm_objects_detect_device(det._h, n, buf, pitch, fstride, rng, (C.c_int * 3)(*cls), nr, K, 1, 1, masks, mpitch, mplane,
                                            buf + 32768, 16, buf + 60000, buf + 62000, None)

    assert call() == 0 and call(n=0) == 0
    assert call(cls=(0, 1, 2), nr=3, K=3) == BAD_PARAM                      # more classes than the handle was made for
    assert call(pitch=3 * W - 1) == BAD_SIZE and call(mpitch=W - 1) == BAD_SIZE
    assert call(fstride=3 * W * H - 1) == BAD_SIZE and call(mplane=W * H - 1) == BAD_SIZE
    assert call(n=1, fstride=0) == 0 and call(n=1, cls=(0, 0), K=1, mplane=0) == 0      # no second frame, no second plane
    assert call(masks=None, mpitch=0, mplane=0) == 0
    torch.cuda.synchronize()
    det.close()


# ---- the whole per-frame chain ---------------------------------------------------------------------------------------
BLUE_LOW, BLUE_HIGH = (110, 150, 0), (130, 255, 255)


def two_colour_scene(synth, c, D):
    """rectify_util.red_scene with the objects of the right half turned blue (R and B swapped) in both views."""
    left, right = ru.red_scene(synth, 1, c["W"], c["H"], D)
    for img in (left, right):
        half = img[:, c["W"] // 2:]
        red = (half[..., 0] > half[..., 1])
        half[red] = half[red][:, ::-1]
    return left, right


@pytest.fixture(scope="module")
def chain(pkg, oracle):
    c, maps = ru.maps(oracle, "320x240")
    x, y, rw, rh = c["roi"]
    rect = pkg.HIPRectifier(*maps, roi=c["roi"])
    m = pkg.HIPMatcher(numOfDisparities=32, blockSize=7, width=rw, height=rh)
    yield c, maps, rect, m
    m.close(); rect.close()


def test_chain_with_one_class_is_estimate_frame(pkg, synth, chain):
    c, maps, rect, m = chain
    left, right = ru.red_scene(synth, 1, c["W"], c["H"], 32)
    det = pkg.HIPObjectDetector(c["roi"][2], c["roi"][3])
    boxes, mean, cnt, disp = pkg.estimate_frame(m, rect, det, left, right, c["Q"], min_area=40, want_disp=True)
    objs, mean2, cnt2, disp2 = pkg.estimate_frame_classes(m, rect, det, left, right, c["Q"], [(pkg.objects.HSV_LOW, pkg.objects.HSV_HIGH)],
                                                          min_area=40, want_disp=True)
    assert len(boxes) >= 2 and objs == [b + (0,) for b in boxes]
    assert np.array_equal(cnt, cnt2) and cnt.sum() > 0 and np.array_equal(mean, mean2) and np.array_equal(disp, disp2)
    # the single-frame calls on this handle still say what a fresh handle says
    fresh = pkg.HIPObjectDetector(c["roi"][2], c["roi"][3])
    again = pkg.estimate_frame(m, rect, det, left, right, c["Q"], min_area=40, want_disp=True)
    new = pkg.estimate_frame(m, rect, fresh, left, right, c["Q"], min_area=40, want_disp=True)
    for a, b, w in zip(again, new, (boxes, mean, cnt, disp)):
        assert np.array_equal(a, b) and np.array_equal(a, w)
    det.close(); fresh.close()


def test_chain_with_two_classes(pkg, oracle, synth, chain):
    c, maps, rect, m = chain
    D, w, min_area = 32, 7, 40
    left, right = two_colour_scene(synth, c, D)
    ranges = [(oracle.HSV_LOW, oracle.HSV_HIGH), (BLUE_LOW, BLUE_HIGH)]
    rw, rh = c["roi"][2], c["roi"][3]
    det = pkg.HIPObjectDetector(rw, rh, max_classes=2)
    fresh = pkg.HIPObjectDetector(rw, rh)
    col = oracle.rectify_rgb(left, maps[0], maps[1], c["roi"])
    before = det.detect(col, min_area=min_area)
    objs, mean, cnt, disp = pkg.estimate_frame_classes(m, rect, det, left, right, c["Q"], ranges, min_area=min_area, want_disp=True)
    # the same chain on the CPU oracle
    gl = oracle.rectify_gray(left, maps[0], maps[1], c["roi"]); gr = oracle.rectify_gray(right, maps[2], maps[3], c["roi"])
    want = ref.detect(oracle, col, ranges, None, min_area, True, oracle.morph_open_close)
    assert min(want["counts"]) >= 1 and objs == want["objects"][:64]
    want_disp = oracle.bm_compute(gl, gr, numDisparities=D, blockSize=w, roi1=want["roi"], nthreads=8)
    assert np.array_equal(disp, want_disp)
    wm, wc = ref.depth(oracle, want_disp, c["Q"], want["masks"], want["objects"], 64)
    assert np.array_equal(cnt, wc) and all(wc[[o[4] == k for o in objs]].sum() > 0 for k in (0, 1))
    assert np.allclose(mean, wm, rtol=1e-9, atol=0)
    # rtdm_objects_detect and rtdm_estimate_frame on the same handle, before and after, are a fresh handle's
    after = det.detect(col, min_area=min_area)
    new = fresh.detect(col, min_area=min_area)
    for a, b, n in zip(before, after, new):
        assert np.array_equal(a, b) and np.array_equal(a, n)
    got = pkg.estimate_frame(m, rect, det, left, right, c["Q"], min_area=min_area, want_disp=True)
    new = pkg.estimate_frame(m, rect, fresh, left, right, c["Q"], min_area=min_area, want_disp=True)
    for a, b in zip(got, new):
        assert np.array_equal(a, b)
    assert len(got[0]) == want["counts"][0]
    # a frame without objects of either class: the matcher is skipped
    gray = np.ascontiguousarray(np.stack([left[..., 1]] * 3, -1))
    objs, mean, cnt = pkg.estimate_frame_classes(m, rect, det, gray, gray, c["Q"], ranges)
    assert objs == [] and len(mean) == 0
    det.close(); fresh.close()
