"""Label planes, pixel moments and own-pixel depth on the device (rtdm_objects_detect_labels_device / _batch,
rtdm_depth_objects_labels_device, rtdm_estimator_set_own_pixels; rules L1-L8 of DESIGN.md section 4.17) against
tests/cc_labels_ref.py, the scipy labelling that tests/test_objects_labels_cpu.py anchors to the CPU oracle.

As in tests/test_gpu_objects_raw.py the detector filters with ERODE by a 1x1 RECT (the identity) unless a test says otherwise,
so the planes that are labelled are the planes that were painted.  Labels, moments, objects and pixel counts are compared
exactly; a mean depth is the oracle's sum in another fixed order and is held to 1e-9 relative, the bound section 4.16 uses for
rule D3 (for <= 4e5 same-sign terms reordering a double sum moves it by about 4e-11 relative)."""
import ctypes as C

import numpy as np
import pytest

import cc_cases as cc
import cc_labels_ref as lr
import labels_scene as ls
import objects_batch_ref as ref
import rectify_util as ru

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
LABEL0 = -0x5A5A5A5B                             # 0xA5A5A5A5 as int32: what a label plane holds before a call
NULL, BAD_PARAM, BAD_SIZE = -7, -1, -2
SETTINGS = [(zb, area) for zb in (True, False) for area in (1, 12)]
ONE_RANGE, ONE_CLASS = [ref.R_RED], [0]
Q = ru.calib("320x240")["Q"]
FILTERED = -16


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


@pytest.fixture(scope="module")
def detectors(pkg):
    """one single-class identity detector per frame size, shared by the tests of this module"""
    made = {}

    def get(W, H):
        if (W, H) not in made:
            made[(W, H)] = raw_detector(pkg, W, H)
        return made[(W, H)]
    yield get
    for d in made.values():
        d.close()


def prepare(rgbs, K, capacity, labels=True, stats=True, pad=(0, 0)):
    """The device tensors of one call: the frames, and outputs that start as sentinels.  pad: extra (columns, rows) of every
    label plane that no call may touch."""
    import torch
    n, H, W, _ = rgbs.shape
    t = dict(rgb=torch.from_numpy(np.ascontiguousarray(rgbs)).cuda(), capacity=capacity,
             objects=torch.full((n, capacity * 32), SENTINEL, dtype=torch.uint8, device="cuda"),
             counts=torch.full((n, K), -7, dtype=torch.int32, device="cuda"),
             rois=torch.full((n, 4), -7, dtype=torch.int32, device="cuda"),
             masks=torch.full((n, K, H, W), SENTINEL, dtype=torch.uint8, device="cuda"), labels=None, stats=None)
    if labels:
        t["label_buf"] = torch.full((n, K, H + pad[1], W + pad[0]), LABEL0, dtype=torch.int32, device="cuda")
        t["labels"] = t["label_buf"][:, :, :H, :W]
    if stats:
        t["stats"] = torch.full((n, capacity * 48), SENTINEL, dtype=torch.uint8, device="cuda")
    return t


def issue(det, t, ranges, classes, min_area, zero_border):
    det.detect_labels_device(t["rgb"], ranges, classes, t["objects"], t["counts"], t["rois"], d_masks=t["masks"], d_labels=t["labels"],
                             d_stats=t["stats"], min_area=min_area, zero_border=zero_border, capacity=t["capacity"])


def host(pkg, t):
    import torch
    torch.cuda.synchronize()
    n = t["objects"].shape[0]
    out = dict(objects=t["objects"].cpu().numpy().view(pkg.OBJECT_DTYPE).reshape(n, -1), counts=t["counts"].cpu().numpy(),
               rois=t["rois"].cpu().numpy(), masks=t["masks"].cpu().numpy(), labels=None, stats=None)
    if t["labels"] is not None:
        out["labels"] = t["labels"].cpu().numpy()
        out["label_buf"] = t["label_buf"].cpu().numpy()
    if t["stats"] is not None:
        out["stats"] = t["stats"].cpu().numpy().view(pkg.STATS_DTYPE).reshape(n, -1)
    return out


def run(pkg, det, rgbs, ranges=ONE_RANGE, classes=ONE_CLASS, capacity=9000, min_area=1, zero_border=True, **kw):
    import torch
    t = prepare(rgbs, max(classes) + 1, capacity, **kw)
    torch.cuda.synchronize()
    issue(det, t, ranges, classes, min_area, zero_border)
    return host(pkg, t)


def stats_rows(st):
    return np.stack([st[m] for m in lr.MOMENTS], -1)


def check_frame(got, f, want, capacity, what=""):
    """Frame f of a device result against cc_labels_ref.frame: L1, L2 and the object list they index."""
    stored = want["stored"]
    assert stored == min(len(want["objects"]), capacity)
    assert got["counts"][f].tolist() == want["counts"], (what, f)
    o = got["objects"][f]
    have = list(zip(o["x"][:stored].tolist(), o["y"][:stored].tolist(), o["width"][:stored].tolist(), o["height"][:stored].tolist(),
                    o["cls"][:stored].tolist()))
    assert have == want["objects"][:stored], (what, f)
    assert o["first_pixel"][:stored].tolist() == want["first_pixels"][:stored], (what, f)
    assert o[stored:].tobytes() == bytes([SENTINEL]) * (32 * (len(o) - stored)), "objects past the stored ones were written"
    if got["labels"] is not None:
        bad = np.argwhere(got["labels"][f] != want["labels"])
        assert len(bad) == 0, (what, f, len(bad), bad[:4].tolist())
    if got["stats"] is not None:
        assert np.array_equal(stats_rows(got["stats"][f][:stored]), want["stats"]), (what, f)
        assert got["stats"][f][stored:].tobytes() == bytes([SENTINEL]) * (48 * (capacity - stored)), "moments past the stored ones were written"


SMALL = [n for n in cc.NAMES if n.split("/")[0].endswith("-64x64")]
LARGE = ["dots-257x131", "quilt5-384x384", "border-300x70", "rings_cut_outer2-257x131"]
WIDE = ["wide-%s" % s for s in ("8192x4", "8191x3", "255x5", "256x5", "257x5", "511x5", "513x5", "1025x5", "1x40", "40x1")]


@pytest.mark.parametrize("name", SMALL + LARGE + WIDE)
def test_labels_and_moments_are_exact(pkg, detectors, name):
    m = cc.BY_NAME[name]
    H, W = m.shape
    det = detectors(W, H)
    rgbs = cc.paint(m)[None]
    for zb, area in SETTINGS:
        want = lr.frame([m], area, zb, 9000)
        got = run(pkg, det, rgbs, min_area=area, zero_border=zb)
        assert np.array_equal(got["masks"][0, 0], m)
        check_frame(got, 0, want, 9000, (name, zb, area))
    if name == "dots-257x131":
        assert want["counts"] == [0] and lr.frame([m], 1, True)["counts"] == [8320]       # the last setting keeps none, the first all


def test_capacity_below_the_total(pkg, detectors):
    m = cc.BY_NAME["dots-64x64"]
    det = detectors(64, 64)
    whole = lr.frame([m], 1, True)
    assert len(whole["objects"]) > 400
    want = lr.frame([m], 1, True, 100)
    assert want["stored"] == 100 and set(np.unique(want["labels"]).tolist()) == set(range(101))
    got = run(pkg, det, cc.paint(m)[None], capacity=100)
    check_frame(got, 0, want, 100)                       # objects and moments beyond the stored ones keep their sentinel
    unstored = (whole["labels"][0] > 100)
    assert unstored.sum() > 300 and (got["labels"][0, 0][unstored] == 0).all()
    assert got["counts"][0].tolist() == [len(whole["objects"])]          # the count is never clipped
    got = run(pkg, det, cc.paint(m)[None], capacity=0)
    assert not got["labels"].any() and got["stats"].size == 0


@pytest.mark.parametrize("pad", [(7, 1), (5, 2)])
def test_padded_label_pitch_and_plane_stride(pkg, oracle, pad):
    """257 ints and 7 of padding make rows of 1056 bytes: 16-byte stores with a tail of one int; 5 of padding make rows of
    1048 bytes: dword stores.  Nothing outside the 257 ints of a row is written."""
    W, H = cc.BIG
    planes = [cc.BY_NAME["%s-%dx%d" % (n, W, H)] for n in ("noise45", "rings_cut2", "stairs", "spiral")]
    rgbs = np.stack([ref.paint2(planes[0], planes[1]), ref.paint2(planes[2], planes[3])])
    det = raw_detector(pkg, W, H, max_batch=2, max_classes=2)
    got = run(pkg, det, rgbs, ref.TWO_RANGES, ref.TWO_CLASSES, capacity=3000, pad=pad)
    assert got["label_buf"].strides[2] == (W + pad[0]) * 4
    for f in range(2):
        masks = ref.detect(oracle, rgbs[f], ref.TWO_RANGES, ref.TWO_CLASSES, 1, True)["masks"]
        check_frame(got, f, lr.frame(masks, 1, True, 3000), 3000)
    assert (got["label_buf"][:, :, :, W:] == LABEL0).all() and (got["label_buf"][:, :, H:, :] == LABEL0).all()
    det.close()


@pytest.fixture(scope="module")
def shared_pixels():
    """three different frames whose two classes share pixels (green = both), and what the reference says of each"""
    W, H = cc.BIG
    names = ["noise45", "rings_cut2", "border", "stairs", "rings_cut_outer2", "noise60"]
    planes = [cc.BY_NAME["%s-%dx%d" % (n, W, H)] for n in names]
    assert all((planes[2 * f] & planes[2 * f + 1]).any() for f in range(3))
    rgbs = np.stack([ref.paint2(planes[2 * f], planes[2 * f + 1]) for f in range(3)])
    return rgbs, [lr.frame([planes[2 * f], planes[2 * f + 1]], 1, True, 3000) for f in range(3)]


def test_two_classes_sharing_pixels_whatever_the_batch(pkg, shared_pixels):
    """L1 / L2 on two planes per frame, and L4: the same frame gives the same bytes in a batch of three, alone, in a call of
    five frames on a handle that takes two, on a handle of another max_batch, and the second time."""
    rgbs, want = shared_pixels
    kw = dict(ranges=ref.TWO_RANGES, classes=ref.TWO_CLASSES, capacity=3000)
    det = raw_detector(pkg, *cc.BIG, max_batch=4, max_classes=2)
    base = run(pkg, det, rgbs, **kw)
    for f in range(3):
        check_frame(base, f, want[f], 3000)
        assert want[f]["counts"][0] > 0 and want[f]["counts"][1] > 0
    again = run(pkg, det, rgbs, **kw)
    alone = [run(pkg, det, rgbs[f:f + 1], **kw) for f in range(3)]
    det.close()
    det = raw_detector(pkg, *cc.BIG, max_batch=2, max_classes=2)
    order = [2, 0, 1, 0, 2]                              # n = 5 > max_batch = 2: three chunks, every frame at another position
    chunked = run(pkg, det, rgbs[order], **kw)
    det.close()
    keys = ("objects", "counts", "rois", "masks", "labels", "stats")
    for k in keys:
        assert again[k].tobytes() == base[k].tobytes(), k
        for f in range(3):
            assert alone[f][k][0].tobytes() == base[k][f].tobytes(), (k, f)
        for pos, f in enumerate(order):
            assert chunked[k][pos].tobytes() == base[k][f].tobytes(), (k, pos)


def test_output_combinations(pkg, shared_pixels):
    import torch
    rgbs, want = shared_pixels
    kw = dict(ranges=ref.TWO_RANGES, classes=ref.TWO_CLASSES, capacity=3000)
    det = raw_detector(pkg, *cc.BIG, max_batch=4, max_classes=2)
    both = run(pkg, det, rgbs, **kw)
    only_labels = run(pkg, det, rgbs, stats=False, **kw)
    only_stats = run(pkg, det, rgbs, labels=False, **kw)
    neither = run(pkg, det, rgbs, labels=False, stats=False, **kw)
    assert only_labels["stats"] is None and only_stats["labels"] is None
    assert only_labels["labels"].tobytes() == both["labels"].tobytes() and only_stats["stats"].tobytes() == both["stats"].tobytes()
    for f in range(3):
        check_frame(only_labels, f, want[f], 3000); check_frame(only_stats, f, want[f], 3000)
    # L3: with neither, the bytes of rtdm_objects_detect_device on the same input, untouched tails included
    t = prepare(rgbs, 2, 3000, labels=False, stats=False)
    torch.cuda.synchronize()
    det.detect_device(t["rgb"], ref.TWO_RANGES, ref.TWO_CLASSES, t["objects"], t["counts"], t["rois"], d_masks=t["masks"], min_area=1,
                      capacity=3000)
    plain = host(pkg, t)
    for k in ("objects", "counts", "rois", "masks"):
        assert neither[k].tobytes() == plain[k].tobytes(), k
        assert both[k].tobytes() == plain[k].tobytes(), k                  # ... and the new outputs change none of the old ones
    assert (plain["objects"][0][int(plain["counts"][0].sum()):].view(np.uint8) == SENTINEL).all()
    # the host entry point says the same
    objs, rois, counts, masks, labels, stats = det.detect_labels(rgbs, ref.TWO_RANGES, ref.TWO_CLASSES, min_area=1, capacity=3000)
    assert labels.tobytes() == both["labels"].tobytes() and masks.tobytes() == both["masks"].tobytes()
    for f in range(3):
        assert objs[f] == want[f]["objects"][:want[f]["stored"]] and np.array_equal(stats_rows(stats[f]), want[f]["stats"])
        assert np.allclose(pkg.centroids(stats[f]), want[f]["stats"][:, 1:3] / want[f]["stats"][:, :1], rtol=0, atol=0)
    objs2, _, _, m2, l2, s2 = det.detect_labels(rgbs, ref.TWO_RANGES, ref.TWO_CLASSES, min_area=1, capacity=3000, want_masks=False,
                                                want_labels=False, want_stats=False)
    assert objs2 == objs and m2 is None and l2 is None and s2 is None
    det.close()


def test_refusals_that_need_the_handle(pkg):
    import torch
    B = pkg.binding
    L = B.lib()
    W, H = 40, 12
    det = raw_detector(pkg, W, H, max_batch=2, max_classes=2)
    buf = torch.zeros(1 << 17, dtype=torch.uint8, device="cuda").data_ptr()
    rng = (B.HsvRange * 2)(*[B.HsvRange((C.c_int * 3)(0, 0, 0), (C.c_int * 3)(255, 255, 255)) for _ in range(2)])
    lab, st = buf + 65536, buf + 40000

    def call(n=2, cls=(0, 1), K=2, pitch=3 * W, labels=lab, lpitch=4 * W, lplane=4 * W * H, stats=st):
        return L.rtdm_objects_detect_labels_device(det._h, n, buf, pitch, 3 * W * H, rng, (C.c_int * 2)(*cls), 2, K, 1, 1, None, 0, 0,
                                                   buf + 32768, 16, buf + 60000, buf + 62000, labels, lpitch, lplane, stats, None)

    assert call() == 0 and call(n=0) == 0
    assert call(pitch=3 * W - 1) == BAD_SIZE                                # the detector's own refusals come first ...
    assert call(pitch=3 * W - 1, lpitch=3) == BAD_SIZE
    assert call(lpitch=4 * W - 4) == BAD_SIZE and call(lpitch=4 * W + 2, lplane=(4 * W + 2) * H) == BAD_SIZE
    assert call(lplane=4 * W * H - 4) == BAD_SIZE and call(lplane=4 * W * H + 2) == BAD_SIZE
    assert call(n=1, cls=(0, 0), K=1, lplane=0) == 0                        # no second plane: the stride is free ...
    assert call(n=1, cls=(0, 0), K=1, lplane=2) == BAD_SIZE                 # ... but stays a multiple of 4
    for off in (1, 2, 3):
        assert call(labels=lab + off) == BAD_SIZE
    for off in (1, 4, 7):
        assert call(stats=st + off) == BAD_SIZE
    assert call(labels=None, lpitch=0, lplane=0) == 0 and call(stats=None) == 0
    assert call(labels=None, lpitch=3, lplane=1, stats=None) == 0           # what is said of absent planes is not looked at
    torch.cuda.synchronize()
    det.close()


# ---- own-pixel depth ----------------------------------------------------------------------------------------------------------
def ramp_map(W, H, seed):
    """a x16 map: a ramp in x and y, a tenth of the pixels invalid -- and those are the frame's minimum --, a few more of
    them in a block"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    disp = (40 + 2 * xx + 3 * yy + rng.integers(0, 16, (H, W))).astype(np.int16)
    disp[rng.random((H, W)) < 0.1] = FILTERED
    disp[H // 3:H // 3 + 4, W // 4:W // 4 + 9] = FILTERED
    return disp


def depth_both(pkg, t, disp, cap):
    """the two depth calls on the device lists of t -> ((mean, npix) of the labels form, (mean, npix) of the mask form)"""
    import torch
    d_disp = torch.from_numpy(disp).cuda()
    out = []
    for fn, planes in ((pkg.depth_objects_labels_device, t["labels"]), (pkg.depth_objects_device, t["masks"])):
        d_mean = torch.full((disp.shape[0], cap), -777.0, dtype=torch.float64, device="cuda")
        d_npix = torch.full((disp.shape[0], cap), -777, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ws = fn(d_disp, Q, planes, t["objects"], t["counts"], d_mean, d_npix, capacity=cap)
        torch.cuda.synchronize()
        del ws
        out.append((d_mean.cpu().numpy(), d_npix.cpu().numpy()))
    return out


@pytest.mark.parametrize("name,kept", [("rings_cut_outer2-257x131", 17), ("noise45-257x131", 145)])
def test_depth_over_own_pixels(pkg, oracle, detectors, name, kept):
    import torch
    m = cc.BY_NAME[name]
    H, W = m.shape
    cap = 160
    want = lr.frame([m], 1, True, cap)
    assert want["stored"] == kept
    dirty = lr.contaminated([m], want["labels"], want["objects"], kept)
    t = prepare(cc.paint(m)[None], 1, cap)
    torch.cuda.synchronize()
    issue(detectors(W, H), t, ONE_RANGE, ONE_CLASS, 1, True)
    check_frame(host(pkg, t), 0, want, cap)
    disp = ramp_map(W, H, 5)[None]
    (mean, npix), (mean_mask, npix_mask) = depth_both(pkg, t, disp, cap)
    wm, wn = lr.depth_own(oracle, disp[0], Q, want["labels"], want["objects"], kept)
    assert np.array_equal(npix[0, :kept], wn) and (wn > 0).sum() >= kept * 9 // 10
    np.testing.assert_allclose(mean[0, :kept], wm, rtol=1e-9, atol=0)
    assert (npix[0, kept:] == -777).all() and (mean[0, kept:] == -777.0).all()
    clean = [i for i in range(kept) if not dirty[i]]
    assert len(clean) == (0 if name.startswith("rings") else 125)
    # L5: an object whose box holds no foreign foreground gets the same bits from both calls ...
    assert mean[0, clean].tobytes() == mean_mask[0, clean].tobytes() and npix[0, clean].tobytes() == npix_mask[0, clean].tobytes()
    # ... and the others are what the mask form gets wrong: it counts the neighbours' pixels too
    bad = [i for i in range(kept) if dirty[i]]
    assert (npix_mask[0, bad] >= npix[0, bad]).all() and (npix_mask[0, bad] > npix[0, bad]).sum() >= len(bad) // 2
    mm, mn = ref.depth(oracle, disp[0], Q, [m], want["objects"], cap, max_regions=cap)
    assert np.array_equal(npix_mask[0, :kept], mn)


def test_hostile_lists_and_hostile_labels(pkg, oracle):
    """L6 / D4: lists that name no plane, no pixel or too much of them, counts below zero, and label planes full of values that
    are nobody's -- npix 0 and mean 0.0 where nothing can be measured, the clipped part where something can, no sentinel touched."""
    import torch
    W, H, K, cap = 300, 9, 2, 16
    big = 2 ** 31 - 1
    rng = np.random.default_rng(3)
    labels = rng.choice(np.array([0, 1, 2, 3, 11, -1, big, -big - 1, 1 << 20], np.int32), (2, K, H, W))
    disp = np.stack([ramp_map(W, H, 8), ramp_map(W, H, 9)])
    f0 = [(-5, -2, 20, 6, 0), (290, 5, 50, 50, 1), (10, 2, -4, 3, 0), (400, 2, 5, 5, 0), (5, 20, 3, 3, 1), (3, 3, 10, 4, 9),
          (3, 3, 10, 4, -1), (big - 40, 1, big - 40, 3, 0), (-big - 1, 0, big, 5, 1), (-big - 1, -big - 1, big, big, 0),
          (10, 1, big, big, 1), (0, 0, 0, 0, 0)]
    f1 = [(-1, -1, W + 2, H + 2, 1)]
    lists = [f0, f1]
    counts = np.array([[-5, len(f0)], [1, -(2 ** 31)]], np.int32)
    obj = np.full((2, cap * 32), SENTINEL, np.uint8)
    rec = obj.view(pkg.OBJECT_DTYPE).reshape(2, cap)
    for f, lst in enumerate(lists):
        for i, o in enumerate(lst):
            rec[f, i] = (o[0], o[1], o[2], o[3], o[4], 0, (0, 0))
    d_mean = torch.full((2, cap), -777.0, dtype=torch.float64, device="cuda")
    d_npix = torch.full((2, cap), -777, dtype=torch.int32, device="cuda")
    d_labels, d_obj = torch.from_numpy(labels).cuda(), torch.from_numpy(obj).cuda()
    torch.cuda.synchronize()
    ws = pkg.depth_objects_labels_device(torch.from_numpy(disp).cuda(), Q, d_labels, d_obj, torch.from_numpy(counts).cuda(), d_mean, d_npix,
                                         capacity=cap)
    torch.cuda.synchronize()
    del ws
    mean, npix = d_mean.cpu().numpy(), d_npix.cpu().numpy()
    for f, lst in enumerate(lists):
        stored = min(int(np.maximum(counts[f], 0).sum()), cap)
        assert stored == len(lst)
        for i, o in enumerate(lst):
            box = lr.clipped(o, W, H)
            if box is None or not 0 <= o[4] < K:
                assert npix[f, i] == 0 and mean[f, i] == 0.0, (f, i)
                continue
            own = ((labels[f, o[4]] == i + 1) * 255).astype(np.uint8)
            wm, wn = oracle.depth_stats(disp[f], Q, own, [box])
            assert npix[f, i] == wn[0], (f, i)
            np.testing.assert_allclose(mean[f, i], wm[0], rtol=1e-9, atol=0)
        assert (npix[f, stored:] == -777).all() and (mean[f, stored:] == -777.0).all()
    assert npix[0, 0] > 0 and npix[0, 1] > 0 and npix[1, 0] > 0            # labels 1 and 2 do occur in the clipped boxes
    assert npix[0, 10] > 0                                                  # ... and 11 in the box that runs off to the right
    assert [i for i in range(len(f0)) if lr.clipped(f0[i], W, H) is None or not 0 <= f0[i][4] < K] == [2, 3, 4, 5, 6, 7, 8, 9, 11]


# ---- the estimator ------------------------------------------------------------------------------------------------------------
CAP = 16


def make_chain(pkg, c, maps, **kw):
    rw, rh = c["roi"][2], c["roi"][3]
    rect = pkg.HIPRectifier(*maps, roi=c["roi"])
    m = pkg.HIPMatcher(numOfDisparities=ls.D, blockSize=ls.BLOCK, width=rw, height=rh, max_batch=2)
    det = pkg.HIPObjectDetector(rw, rh, max_batch=2, max_classes=1)          # the default open + close
    return [pkg.HIPEstimator(m, rect, det, max_batch=2, capacity=CAP, **kw), det, m, rect]


def estimate(est, c, oracle, lefts, rights):
    disp = np.full((len(lefts), c["roi"][3], c["roi"][2]), 0x5A5A, np.int16)
    return est.estimate(lefts, rights, c["Q"], ls.ranges(oracle), min_area=ls.MIN_AREA, disp=disp)


def test_estimator_own_pixels(pkg, oracle):
    c, maps = ru.maps(oracle, "320x240")
    left, right = ls.pair(c)
    lefts, rights = np.stack([left] * 3), np.stack([right] * 3)              # three frames on a chunk of two
    # the reference chain
    want = ls.detect(oracle, c, maps, left)
    fr = lr.frame(want["masks"], ls.MIN_AREA, True, CAP)
    gl = oracle.rectify_gray(left, maps[0], maps[1], c["roi"]); gr = oracle.rectify_gray(right, maps[2], maps[3], c["roi"])
    wdisp = oracle.bm_compute(gl, gr, numDisparities=ls.D, blockSize=ls.BLOCK, roi1=want["roi"], nthreads=8)
    own_mean, own_npix = lr.depth_own(oracle, wdisp, c["Q"], fr["labels"], fr["objects"], 2)
    cls_mean, cls_npix = ref.depth(oracle, wdisp, c["Q"], want["masks"], want["objects"], CAP)
    assert own_npix[1] > 1000 and cls_npix[1] > own_npix[1] + 300 and own_npix[0] == cls_npix[0] > 300
    assert abs(own_mean[1] - cls_mean[1]) > 1.0                              # the square pulls the L's mean by centimetres

    never = make_chain(pkg, c, maps)                                       # a handle that never heard of the switch
    plain = estimate(never[0], c, oracle, lefts, rights)
    for h in never:
        h.close()
    chain = make_chain(pkg, c, maps, own_pixels=False)
    est = chain[0]
    assert est.own_pixels is False
    off = estimate(est, c, oracle, lefts, rights)
    est.own_pixels = True
    assert est.own_pixels is True
    on = estimate(est, c, oracle, lefts, rights)
    est.own_pixels = False
    assert est.own_pixels is False
    off_again = estimate(est, c, oracle, lefts, rights)
    for h in chain:
        h.close()
    born_on = make_chain(pkg, c, maps, own_pixels=True)
    assert born_on[0].own_pixels is True
    on2 = estimate(born_on[0], c, oracle, lefts, rights)
    for h in born_on:
        h.close()

    def same(a, b):
        assert a[0] == b[0] and a[1].tobytes() == b[1].tobytes() and a[4].tobytes() == b[4].tobytes()
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a[2], b[2])) and all(x.tobytes() == y.tobytes() for x, y in zip(a[3], b[3]))

    same(off, plain); same(off_again, plain); same(on2, on)
    for f in range(3):
        # objects, counts and maps are unaffected by the switch
        assert on[0][f] == off[0][f] == want["objects"] and on[1][f].tolist() == off[1][f].tolist() == [2]
        assert np.array_equal(on[4][f], wdisp) and np.array_equal(off[4][f], wdisp)
        assert np.array_equal(on[3][f], own_npix) and np.array_equal(off[3][f], cls_npix)
        np.testing.assert_allclose(on[2][f], own_mean, rtol=1e-9, atol=0)
        np.testing.assert_allclose(off[2][f], cls_mean, rtol=1e-9, atol=0)
        # the two settings differ for the L-shaped object and agree, bit for bit, for the square
        assert on[3][f][1] < off[3][f][1] and abs(on[2][f][1] - off[2][f][1]) > 1.0
        assert on[3][f][0] == off[3][f][0] and on[2][f][0].tobytes() == off[2][f][0].tobytes()


def test_estimator_own_pixels_on_the_device_form(pkg, oracle):
    import torch
    c, maps = ru.maps(oracle, "320x240")
    left, right = ls.pair(c)
    chain = make_chain(pkg, c, maps, own_pixels=True)
    est = chain[0]
    want = estimate(est, c, oracle, left[None], right[None])
    d_obj = torch.full((1, CAP * 32), SENTINEL, dtype=torch.uint8, device="cuda")
    d_cnt = torch.zeros((1, 1), dtype=torch.int32, device="cuda")
    d_mean = torch.full((1, CAP), -777.0, dtype=torch.float64, device="cuda")
    d_npix = torch.full((1, CAP), -777, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    est.estimate_device(torch.from_numpy(left[None]).cuda(), torch.from_numpy(right[None]).cuda(), c["Q"], ls.ranges(oracle), None, d_obj,
                        d_cnt, d_mean, d_npix, min_area=ls.MIN_AREA)
    torch.cuda.synchronize()
    assert d_cnt.cpu().numpy().tolist() == [[2]]
    assert d_npix.cpu().numpy()[0, :2].tobytes() == want[3][0].tobytes() and d_mean.cpu().numpy()[0, :2].tobytes() == want[2][0].tobytes()
    assert (d_npix.cpu().numpy()[0, 2:] == -777).all()
    for h in chain:
        h.close()
