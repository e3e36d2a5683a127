"""Per-object measurements on the device (rtdm_objects_measure_device, rtdm_estimate_batch_measured / _device; rules G1-G10 of
DESIGN.md section 4.18) against tests/measure_ref.py, the numpy restatement that tests/test_measure_cpu.py anchors to
per-object Python loops.

The device lists come from the raw detector (ERODE by a 1x1 RECT, the identity), as in tests/test_gpu_objects_labels.py, whose
helpers and ramp map are used here.  npix, nplane, the quantiles and the extent are compared bytewise.  A centre is the
reference's math.fsum mean in another fixed order: it is held to npix * 2^-52 * sum |v_j| / npix (measure_ref.measure_with_bound), the
bound of any summation order, doubled for the division."""
import numpy as np
import pytest

import cc_cases as cc
import cc_labels_ref as lr
import d3_walk_model as d3
import labels_scene as ls
import measure_ref as mr
import rectify_util as ru
import xyz_ref as xr
from test_gpu_objects_labels import ONE_CLASS, ONE_RANGE, SENTINEL, check_frame, depth_both, host, issue, prepare, ramp_map, raw_detector

pytestmark = pytest.mark.gpu

Q = np.array(ru.calib("320x240")["Q"], np.float64)
GUARD = 64
MODES = (xr.ROUNDED, xr.FIXED16)


@pytest.fixture(scope="module")
def pkg():
    import torch                         # torch first: it brings its own HIP runtime and must initialise before ours
    assert torch.cuda.is_available()
    from conftest import load
    return load()


@pytest.fixture(scope="module")
def detected(pkg):
    """name -> (device tensors of the raw detector's call on that mask, their host copies), made once per mask"""
    import torch
    made, dets = {}, {}

    def get(name, cap=9000):
        if (name, cap) not in made:
            m = cc.BY_NAME[name]
            H, W = m.shape
            if (W, H) not in dets:
                dets[(W, H)] = raw_detector(pkg, W, H)
            t = prepare(cc.paint(m)[None], 1, cap)
            torch.cuda.synchronize()
            issue(dets[(W, H)], t, ONE_RANGE, ONE_CLASS, 1, True)
            h = host(pkg, t)
            check_frame(h, 0, lr.frame([m], 1, True, cap), cap, name)
            made[(name, cap)] = (t, h)
        return made[(name, cap)]
    yield get
    for d in dets.values():
        d.close()


def measure(pkg, disp, q, d_planes, d_objects, d_counts, cap, labels, params=None):
    """one call -> MEASURE records n x cap from a buffer of sentinels with 64 guard bytes either side, which must survive"""
    import torch
    n = disp.shape[0]
    buf = torch.full((GUARD + n * cap * 88 + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_meas = buf[GUARD:GUARD + n * cap * 88].view(n, cap * 88)
    d_disp = torch.from_numpy(np.ascontiguousarray(disp)).cuda()
    torch.cuda.synchronize()
    ws = pkg.objects_measure_device(d_disp, q, d_planes, d_objects, d_counts, d_meas, params=params, labels=labels, capacity=cap)
    torch.cuda.synchronize()
    del ws
    raw = buf.cpu().numpy()
    assert (raw[:GUARD] == SENTINEL).all() and (raw[-GUARD:] == SENTINEL).all(), "guard bytes were written"
    return raw[GUARD:-GUARD].copy().view(pkg.MEASURE_DTYPE).reshape(n, cap)


def compare(got, want, bound, what=""):
    """one frame: got cap records, want the reference's stored ones"""
    stored = len(want)
    assert mr.same_exact(got[:stored], want) is None, (what, mr.same_exact(got[:stored], want))
    err = np.abs(got["mean"][:stored] - want["mean"])
    assert (err <= bound).all(), (what, float(err.max()), np.argwhere(err > bound)[:3].tolist())
    empty = want["npix"] == 0
    assert got["mean"][:stored][empty].tobytes() == bytes(24 * int(empty.sum())), "G8: +0.0"
    assert got[stored:].tobytes() == bytes([SENTINEL]) * (88 * (len(got) - stored)), "records past the stored ones were written"


def reference(disp, q, planes, objects, counts, cap, labels, mode, max_z=1e4, permille=mr.ALL_PERMILLE):
    return mr.measure_with_bound(disp, q, planes, objects, counts, cap, labels, mode, max_z, permille)


def host_objects(h, f=0):
    o = h["objects"][f]
    return list(zip(o["x"].tolist(), o["y"].tolist(), o["width"].tolist(), o["height"].tolist(), o["cls"].tolist()))


def params_of(pkg, mode, max_z=1e4, permille=mr.ALL_PERMILLE):
    return pkg.MeasureParams(disparity_mode=mode, max_z=max_z, permille=permille)


@pytest.mark.parametrize("name,total,least", [("rings_cut_outer2-257x131", 17, 17), ("noise45-257x131", 145, 130), ("dots-257x131", 8320, 7000)])
def test_exact_on_hostile_masks(pkg, detected, name, total, least):
    t, h = detected(name)
    H, W = cc.BY_NAME[name].shape
    disp = ramp_map(W, H, 5)[None]
    objects, counts = host_objects(h), h["counts"][0]
    assert int(counts.sum()) == total
    for mode in MODES:
        for labels in (True, False):
            planes = h["labels"][0] if labels else h["masks"][0]
            want, bound = reference(disp[0], Q, planes, objects, counts, 9000, labels, mode)
            got = measure(pkg, disp, Q, t["labels"] if labels else t["masks"], t["objects"], t["counts"], 9000, labels, params_of(pkg, mode))
            compare(got[0], want, bound, (name, mode, labels))
            assert int((want["npix"] > 0).sum()) >= least
            if labels:                                               # unclipped boxes: the label count is the detector's m00
                assert np.array_equal(got[0]["nplane"][:total], h["stats"][0]["m00"][:total])
    if name.startswith("noise"):
        assert int(want["npix"].max()) > 10000                       # (mask form, FIXED16: the largest component over many bands)
    if name.startswith("dots"):
        one = got[0][:total][got[0]["npix"][:total] == 1]
        assert len(one) >= least and (one["zq"] == one["lo"][:, 2:3]).all() and (one["lo"] == one["hi"]).all()


def test_both_signs_and_non_finite_points(pkg, detected):
    name = "rings_cut_outer2-257x131"
    t, h = detected(name)
    H, W = cc.BY_NAME[name].shape
    disp = ramp_map(W, H, 5)[None]
    q = Q.copy()
    q[3, 3] = -40.0 * q[3, 2]                                        # h3 = 0 at d = 40: Z changes sign there
    objects, counts = host_objects(h), h["counts"][0]
    for mode, nonfinite in ((xr.ROUNDED, 823), (xr.FIXED16, 45)):
        xyz = xr.reproject(disp[0], q, mode, True)
        assert int((~np.isfinite(xyz[..., 2])).sum()) == nonfinite
        for labels in (True, False):
            planes = h["labels"][0] if labels else h["masks"][0]
            want, bound = reference(disp[0], q, planes, objects, counts, 9000, labels, mode)
            assert len(want) == 17 and (want["lo"][:, 2] < 0).all() and (want["hi"][:, 2] > 0).all()
            got = measure(pkg, disp, q, t["labels"] if labels else t["masks"], t["objects"], t["counts"], 9000, labels, params_of(pkg, mode))
            compare(got[0], want, bound, (mode, labels))


def device_lists(pkg, lists, counts, cap):
    """hand-made lists -> (d_objects uint8 [n, cap * 32] with sentinels past the entries, d_counts)"""
    import torch
    n = len(lists)
    obj = np.full((n, cap * 32), SENTINEL, np.uint8)
    rec = obj.view(pkg.OBJECT_DTYPE).reshape(n, cap)
    for f, lst in enumerate(lists):
        for i, o in enumerate(lst):
            rec[f, i] = (o[0], o[1], o[2], o[3], o[4], 0, (0, 0))
    return torch.from_numpy(obj).cuda(), torch.from_numpy(np.asarray(counts, np.int32)).cuda()


def test_lane_layout_and_band_edges(pkg):
    import torch
    W, H = 140, 40
    disp = ramp_map(W, H, 7)
    boxes = []
    for w in (1, 2, 3, 63, 64, 65, 130):
        for hh in (1, 15, 16, 17, 33, 40):
            boxes += [(0, 0, w, hh, 0), (min(7, W - w), min(3, H - hh), w, hh, 0), (W - w, H - hh, w, hh, 0)]
    boxes.append((0, 0, W, H, 0))
    cap = len(boxes)
    assert cap == 127
    # mask form: one frame, every box over a plane that is all foreground
    d_obj, d_cnt = device_lists(pkg, [boxes], [[cap]], cap)
    plane = np.full((1, 1, H, W), 255, np.uint8)
    for mode in MODES:
        want, bound = reference(disp, Q, plane[0], boxes, [cap], cap, False, mode)
        assert (want["nplane"] == [b[2] * b[3] for b in boxes]).all() and (want["npix"] > 0).sum() >= cap - 10
        got = measure(pkg, disp[None], Q, torch.from_numpy(plane).cuda(), d_obj, d_cnt, cap, False, params_of(pkg, mode))
        compare(got[0], want, bound, ("mask", mode))
    # label form: object 0 of a frame owns the label 1, so one box per frame
    some = boxes[3::11] + boxes[-1:]
    n = len(some)
    d_obj, d_cnt = device_lists(pkg, [[b] for b in some], [[1]] * n, 2)
    labels = np.ones((n, 1, H, W), np.int32)
    got = measure(pkg, np.stack([disp] * n), Q, torch.from_numpy(labels).cuda(), d_obj, d_cnt, 2, True, params_of(pkg, xr.FIXED16))
    for f, b in enumerate(some):
        want, bound = reference(disp, Q, labels[f], [b], [1], 2, True, xr.FIXED16)
        compare(got[f], want, bound, ("labels", f))


def plain_q(q22, q23, q32, q33, W, H):
    return np.array([[1, 0, 0, -W / 2], [0, 1, 0, -H / 2], [0, 0, q22, q23], [0, 0, q32, q33]], np.float64)


def test_ties_and_tiny_counts(pkg):
    import torch
    W, H, cap = 70, 20, 8
    FX = params_of(pkg, xr.FIXED16)
    full = torch.full((1, 1, H, W), 255, dtype=torch.uint8, device="cuda")
    boxes = [(1, 1, 64, 18, 0), (3, 2, 5, 17, 0), (0, 0, W, H, 0)]
    d_obj, d_cnt = device_lists(pkg, [boxes], [[3]], cap)

    def run(disp, q, params, d_planes=full, planes=np.full((1, H, W), 255, np.uint8), lst=boxes, obj=d_obj, cnt=d_cnt, counts=(3,)):
        want, bound = reference(disp, q, planes, lst, counts, cap, False, params.disparity_mode, params.max_z)
        got = measure(pkg, disp[None], q, d_planes, obj, cnt, cap, False, params)
        compare(got[0], want, bound)
        return want

    # a constant map (but for the one pixel that is the frame's minimum): every kept Z is one value
    disp = np.full((H, W), 600, np.int16); disp[0, 0] = -16
    for mode in MODES:
        want = run(disp, Q, params_of(pkg, mode))
        assert (want["npix"] == [64 * 18, 5 * 17, W * H - 1]).all()
        assert (want["zq"] == want["lo"][:, 2:3]).all() and (want["lo"][:, 2] == want["hi"][:, 2]).all()
    # Z = 1024 + disp * 2^-13, disp in 0 .. 255: keys that differ in their lowest digit only
    rng = np.random.default_rng(21)
    disp = rng.integers(0, 256, (H, W)).astype(np.int16); disp[0, 0] = -16
    want = run(disp, plain_q(2.0 ** -9, 1024.0, 0.0, 1.0, W, H), FX)
    k = mr.keys(np.concatenate([want["lo"][:, 2], want["hi"][:, 2]]))
    assert (k >> 8 == k[0] >> 8).all() and len(np.unique(k)) > 1 and len(np.unique(want["zq"][2])) >= 4
    # Z = 16 / disp, disp a power of four: keys that differ in their highest digit only
    disp = (4 ** rng.integers(0, 8, (H, W))).astype(np.int16); disp[0, 0] = -16
    want = run(disp, plain_q(0.0, 1.0, 1.0, 0.0, W, H), FX)
    k = mr.keys(np.concatenate([want["lo"][:, 2], want["hi"][:, 2]]))
    assert (k & 0xFFFFFF == k[0] & 0xFFFFFF).all() and len(np.unique(k >> 24)) > 1 and len(np.unique(want["zq"][2])) >= 4
    # objects that keep 0, 1, 2 and 3 pixels of a ramp without invalid values
    yy, xx = np.mgrid[0:H, 0:W]
    disp = (40 + 2 * xx + 3 * yy).astype(np.int16); disp[0, 0] = -16
    plane = np.zeros((1, H, W), np.uint8)
    tiny = [(2, 2, 6, 6, 0), (10, 2, 6, 6, 0), (20, 2, 6, 6, 0), (30, 2, 6, 6, 0)]
    plane[0, 4, 12] = 255
    plane[0, 3, 21] = plane[0, 6, 24] = 255
    plane[0, 2, 30] = plane[0, 2, 35] = plane[0, 7, 33] = 255
    obj, cnt = device_lists(pkg, [tiny], [[4]], cap)
    for mode in MODES:
        want = run(disp, Q, params_of(pkg, mode), torch.from_numpy(plane[None]).cuda(), plane, tiny, obj, cnt, (4,))
        assert want["npix"].tolist() == [0, 1, 2, 3] and want["nplane"].tolist() == [0, 1, 2, 3]
        assert not want[0]["zq"].any() and (want[1]["zq"] == want[1]["lo"][2]).all()


def test_max_z_drops_the_far_pixels(pkg, detected):
    name = "rings_cut_outer2-257x131"
    t, h = detected(name)
    H, W = cc.BY_NAME[name].shape
    disp = ramp_map(W, H, 5)[None]
    objects, counts = host_objects(h), h["counts"][0]
    for labels in (True, False):
        planes = h["labels"][0] if labels else h["masks"][0]
        far, _ = reference(disp[0], Q, planes, objects, counts, 9000, labels, xr.ROUNDED)
        want, bound = reference(disp[0], Q, planes, objects, counts, 9000, labels, xr.ROUNDED, max_z=12.0)
        assert (want["npix"] < far["npix"]).sum() >= 10 and (want["npix"] > 0).sum() >= 10 and (want["hi"][:, 2] <= 12.0).all()
        got = measure(pkg, disp, Q, t["labels"] if labels else t["masks"], t["objects"], t["counts"], 9000, labels,
                      params_of(pkg, xr.ROUNDED, max_z=12.0))
        compare(got[0], want, bound, labels)


def test_hostile_lists_and_hostile_labels(pkg):
    """D4 / L6 with the lists, counts and label values of tests/test_gpu_objects_labels.py::test_hostile_lists_and_hostile_labels"""
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
    d_obj, d_cnt = device_lists(pkg, lists, counts, cap)
    masks = (labels & 0xFF).astype(np.uint8)
    for mode in MODES:
        for lab, planes in ((True, labels), (False, masks)):
            got = measure(pkg, disp, Q, torch.from_numpy(planes).cuda(), d_obj, d_cnt, cap, lab, params_of(pkg, mode))
            for f, lst in enumerate(lists):
                want, bound = reference(disp[f], Q, planes[f], lst, counts[f], cap, lab, mode)
                assert len(want) == len(lst)
                compare(got[f], want, bound, (mode, lab, f))
                nothing = [i for i in range(len(lst)) if lr.clipped(lst[i], W, H) is None or not 0 <= lst[i][4] < K]
                assert got[f][nothing].tobytes() == bytes(88 * len(nothing))                # G8: zeros in every field
                if f == 0:
                    assert nothing == [2, 3, 4, 5, 6, 7, 8, 9, 11]
                    assert want["npix"][0] > 0 and want["npix"][1] > 0 and want["npix"][10] > 0
                else:
                    assert want["npix"][0] > 0


def test_same_bytes_whatever_the_batch_and_the_capacity(pkg, detected):
    import torch
    name = "noise45-257x131"
    t, h = detected(name)
    t2, h2 = detected("rings_cut_outer2-257x131")
    H, W = cc.BY_NAME[name].shape
    disp, other = ramp_map(W, H, 5), ramp_map(W, H, 6)
    P = params_of(pkg, xr.FIXED16)
    base = measure(pkg, disp[None], Q, t["labels"], t["objects"], t["counts"], 9000, True, P)
    again = measure(pkg, disp[None], Q, t["labels"], t["objects"], t["counts"], 9000, True, P)
    assert base.tobytes() == again.tobytes() and (base[0]["npix"][:145] > 0).sum() >= 130
    # the same frame at position 2 of 3
    three = measure(pkg, np.stack([other, other, disp]), Q, torch.cat([t2["labels"], t2["labels"], t["labels"]]),
                    torch.cat([t2["objects"], t2["objects"], t["objects"]]), torch.cat([t2["counts"], t2["counts"], t["counts"]]), 9000, True, P)
    assert three[2].tobytes() == base[0].tobytes() and (three[0]["npix"][:17] > 0).all()
    # capacity 160 in place of 9000
    small = measure(pkg, disp[None], Q, t["labels"], t["objects"][:, :160 * 32].contiguous(), t["counts"], 160, True, P)
    assert small[0][:145].tobytes() == base[0][:145].tobytes()
    masks = measure(pkg, disp[None], Q, t["masks"], t["objects"], t["counts"], 9000, False, P)
    masks160 = measure(pkg, disp[None], Q, t["masks"], t["objects"][:, :160 * 32].contiguous(), t["counts"], 160, False, P)
    assert masks160[0][:145].tobytes() == masks[0][:145].tobytes()


@pytest.mark.parametrize("name,kept", [("rings_cut_outer2-257x131", 17), ("noise45-257x131", 145)])
def test_the_mean_depth_that_ships_says_the_same(pkg, detected, name, kept):
    """ROUNDED and max_z 1e4 are calc_depth's: npix equal, the distance within 2^-22 relative -- the older kernel's Z may differ
    by one float ulp, 2^-23 relative, where the compiler fused what rule X2 keeps apart."""
    t, h = detected(name, 160)
    H, W = cc.BY_NAME[name].shape
    disp = ramp_map(W, H, 5)[None]
    (mean_l, npix_l), (mean_m, npix_m) = depth_both(pkg, t, disp, 160)
    for labels, mean, npix in ((True, mean_l, npix_l), (False, mean_m, npix_m)):
        got = measure(pkg, disp, Q, t["labels"] if labels else t["masks"], t["objects"], t["counts"], 160, labels,
                      params_of(pkg, xr.ROUNDED))[0][:kept]
        assert np.array_equal(got["npix"], npix[0, :kept]) and (got["npix"] > 0).sum() >= kept * 9 // 10
        cm = pkg.distance_cm(got["mean"][:, 2], 25.0)
        assert (np.abs(cm - mean[0, :kept]) <= 2.0 ** -22 * np.abs(mean[0, :kept])).all()


# ---- the estimator ------------------------------------------------------------------------------------------------------------
CAP = 16


def make_chain(pkg, c, maps, **kw):
    rw, rh = c["roi"][2], c["roi"][3]
    rect = pkg.HIPRectifier(*maps, roi=c["roi"])
    m = pkg.HIPMatcher(numOfDisparities=ls.D, blockSize=ls.BLOCK, width=rw, height=rh, max_batch=2)
    det = pkg.HIPObjectDetector(rw, rh, max_batch=2, max_classes=1)          # the default open + close
    return [pkg.HIPEstimator(m, rect, det, max_batch=2, capacity=CAP, **kw), det, m, rect]


@pytest.mark.parametrize("own", [True, False])
def test_estimator_measures_what_the_call_measures(pkg, oracle, own):
    import torch
    c, maps = ru.maps(oracle, "320x240")
    left, right = ls.pair(c)
    lefts, rights = np.stack([left] * 3), np.stack([right] * 3)              # three frames on a chunk of two
    rw, rh = c["roi"][2], c["roi"][3]
    chain = make_chain(pkg, c, maps, own_pixels=own)
    est, det, _, rect = chain
    P = pkg.MeasureParams(disparity_mode=xr.FIXED16, permille=(500, 0, 1000, 100, 900))
    kw = dict(min_area=ls.MIN_AREA)

    def disp0():
        return np.full((3, rh, rw), 0x5A5A, np.int16)

    plain = est.estimate(lefts, rights, c["Q"], ls.ranges(oracle), disp=disp0(), **kw)
    meas = est.estimate(lefts, rights, c["Q"], ls.ranges(oracle), disp=disp0(), measure=P, **kw)
    after = est.estimate(lefts, rights, c["Q"], ls.ranges(oracle), disp=disp0(), **kw)   # an unmeasured call after a measured one
    assert len(plain) == 5 and len(meas) == 6
    for other in (meas, after):
        assert other[0] == plain[0] and other[1].tobytes() == plain[1].tobytes() and other[4].tobytes() == plain[4].tobytes()
        assert all(a.tobytes() == b.tobytes() for a, b in zip(other[2], plain[2])) and all(a.tobytes() == b.tobytes() for a, b in zip(other[3], plain[3]))
    assert plain[1].tolist() == [[2]] * 3
    # the frame's own lists, planes and map through the detector and rtdm_objects_measure_device
    crop = torch.from_numpy(rect.rgb(left)[None]).cuda()
    t = dict(objects=torch.full((1, CAP * 32), SENTINEL, dtype=torch.uint8, device="cuda"), counts=torch.zeros((1, 1), dtype=torch.int32, device="cuda"),
             rois=torch.zeros((1, 4), dtype=torch.int32, device="cuda"), masks=torch.zeros((1, 1, rh, rw), dtype=torch.uint8, device="cuda"),
             labels=torch.zeros((1, 1, rh, rw), dtype=torch.int32, device="cuda"))
    det.detect_labels_device(crop, ls.ranges(oracle), None, t["objects"], t["counts"], t["rois"], d_masks=t["masks"], d_labels=t["labels"],
                             min_area=ls.MIN_AREA, capacity=CAP)
    torch.cuda.synchronize()
    assert t["counts"].cpu().numpy().tolist() == [[2]]
    direct = measure(pkg, meas[4][:1], c["Q"], t["labels"] if own else t["masks"], t["objects"], t["counts"], CAP, own, P)
    assert (direct[0]["npix"][:2] > 300).all()
    for f in range(3):
        assert meas[5][f].dtype == pkg.MEASURE_DTYPE and meas[5][f].tobytes() == direct[0][:2].tobytes(), f
    # the device form: the same records, left on the stream; entries past the stored ones untouched
    n = 3
    d = dict(obj=torch.full((n, CAP * 32), SENTINEL, dtype=torch.uint8, device="cuda"), cnt=torch.zeros((n, 1), dtype=torch.int32, device="cuda"),
             mean=torch.full((n, CAP), -777.0, dtype=torch.float64, device="cuda"), npix=torch.full((n, CAP), -777, dtype=torch.int32, device="cuda"),
             meas=torch.full((n, CAP * 88), SENTINEL, dtype=torch.uint8, device="cuda"))
    torch.cuda.synchronize()
    est.estimate_device(torch.from_numpy(lefts).cuda(), torch.from_numpy(rights).cuda(), c["Q"], ls.ranges(oracle), None, d["obj"], d["cnt"],
                        d["mean"], d["npix"], d_measures=d["meas"], measure=P, **kw)
    torch.cuda.synchronize()
    rec = d["meas"].cpu().numpy().view(pkg.MEASURE_DTYPE).reshape(n, CAP)
    for f in range(n):
        assert rec[f][:2].tobytes() == direct[0][:2].tobytes() and rec[f][2:].tobytes() == bytes([SENTINEL]) * (88 * (CAP - 2))
        assert d["npix"].cpu().numpy()[f, :2].tobytes() == plain[3][f].tobytes() and d["mean"].cpu().numpy()[f, :2].tobytes() == plain[2][f].tobytes()
    # one of the two missing is refused
    B = pkg.binding
    buf = np.zeros(CAP * 88 * 3 + 64, np.uint8)
    args = [est._h, 0, buf.ctypes.data, 3 * c["W"], 3 * c["W"] * c["H"], buf.ctypes.data, 3 * c["W"], 3 * c["W"] * c["H"],
            np.ascontiguousarray(c["Q"], np.float64).ctypes.data_as(B.C.POINTER(B.C.c_double)), None, None, 0, 0, 1, 1, 25.0,
            buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, None, 0, 0]
    assert B.lib().rtdm_estimate_batch_measured(*(args + [B.C.byref(P.c), None])) == -7
    assert B.lib().rtdm_estimate_batch_measured(*(args + [None, buf.ctypes.data])) == -7
    for hnd in chain:
        hnd.close()


@pytest.mark.parametrize("labels", [False, True])
def test_the_walk_of_a_box_is_rule_d3(pkg, labels):
    """D3 bit for bit, as tests/test_gpu_depth_objects.py holds the depth call to it: the three means, the extent and the two
    counts of every box of tests/d3_walk_model.py's scene equal the model's lane-by-lane, band-by-band float64 sums, on values
    whose sums depend on the order (tests/test_d3_walk_model_cpu.py)."""
    import torch
    disp, mask, planes, boxes = d3.scene()
    plane = planes if labels else mask
    k = len(boxes)
    d_obj, d_cnt = device_lists(pkg, [boxes], [[k]], d3.CAP)
    d_plane = torch.from_numpy(plane[None]).cuda()
    for mode in MODES:
        want = d3.measure_model(disp, plane[0], boxes, labels, mode)
        assert k == d3.CAP - 1 and (want["npix"] > 0).sum() >= k - 6 and (want["nplane"] >= want["npix"]).all()
        got = measure(pkg, disp[None], d3.Q, d_plane, d_obj, d_cnt, d3.CAP, labels, params_of(pkg, mode, permille=()))[0]
        for name in ("npix", "nplane", "lo", "hi", "mean"):
            a, b = np.ascontiguousarray(got[name][:k]), np.ascontiguousarray(want[name])
            assert a.tobytes() == b.tobytes(), (mode, name, np.argwhere(a != b)[:8].tolist())
        assert got[k:].tobytes() == bytes([SENTINEL]) * (88 * (d3.CAP - k))
