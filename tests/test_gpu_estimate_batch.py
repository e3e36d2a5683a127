"""The batched loop body (rtdm_estimator_create, rtdm_estimate_batch, rtdm_estimate_batch_device) against
rtdm_estimate_frame_classes on every frame alone and against the CPU oracle chain.  320x240 calibration (crop 233x156), D = 32,
blockSize 7, min_area 40, a red and a blue class.  The batch is six frame pairs: seed 1, seed 2, seed 2 again (equal union box:
the shared matcher launch), a gray pair without objects, seed 3, seed 5.  The matcher takes 2 frames per launch, detector and
estimator 4, so the chunks are 2 frames and n exceeds every batch.  Objects, counts, pixel counts and disparity maps are compared
exactly; the mean depth is the same sum in another fixed order (rtol 1e-9, as tests/test_gpu_depth_objects.py)."""
import numpy as np
import pytest

import estimate_batch_scenes as sc
import rectify_util as ru

pytestmark = pytest.mark.gpu

CAP = 16
ORDER = [1, 2, 2, None, 3, 5]                    # scene seeds; None: the gray pair
GRAY = 3
DISP0 = 0x5A5A                                   # what a disparity frame holds before the call


@pytest.fixture(scope="module")
def pkg():
    import torch                         # torch first: it brings its own HIP runtime and must initialise before ours
    assert torch.cuda.is_available()
    from conftest import load
    return load()


def fresh(pkg, c, maps, matcher_batch=1, detector_batch=1):
    rw, rh = c["roi"][2], c["roi"][3]
    rect = pkg.HIPRectifier(*maps, roi=c["roi"])
    m = pkg.HIPMatcher(numOfDisparities=sc.D, blockSize=sc.BLOCK, width=rw, height=rh, max_batch=matcher_batch)
    det = pkg.HIPObjectDetector(rw, rh, max_batch=detector_batch, max_classes=2)
    return m, rect, det


def close(*handles):
    for h in handles:
        h.close()


def run_batch(world, lefts, rights):
    """estimate() on sentinel disparity frames -> (objects, counts, means, npix, disp)."""
    c = world["c"]
    disp = np.full((len(lefts), c["roi"][3], c["roi"][2]), DISP0, np.int16)
    return world["est"].estimate(lefts, rights, c["Q"], world["ranges"], min_area=sc.MIN_AREA, disp=disp)


@pytest.fixture(scope="module")
def world(pkg, oracle, synth):
    c, maps = ru.maps(oracle, "320x240")
    scenes = {s: sc.two_colour_scene(synth, c, s) for s in (1, 2, 3, 5)}
    scenes[None] = sc.gray_pair(scenes[1][0])
    lefts = np.stack([scenes[s][0] for s in ORDER]); rights = np.stack([scenes[s][1] for s in ORDER])
    m, rect, det = fresh(pkg, c, maps, matcher_batch=2, detector_batch=4)
    est = pkg.HIPEstimator(m, rect, det, max_batch=4, capacity=CAP)
    w = dict(c=c, maps=maps, lefts=lefts, rights=rights, m=m, rect=rect, det=det, est=est, ranges=sc.ranges(oracle))
    w["batch"] = run_batch(w, lefts, rights)
    yield w
    close(est, det, m, rect)


def test_the_scenes_are_what_the_issue_says(oracle, synth):
    c, maps = ru.maps(oracle, "320x240")
    assert c["roi"][2:] == (233, 156)
    found = [sc.detect(oracle, c, maps, sc.two_colour_scene(synth, c, s)[0]) for s in range(1, 7)]
    assert [f["counts"] for f in found] == [[1, 1], [1, 1], [2, 2], [1, 1], [2, 2], [2, 2]]
    assert len({f["roi"] for f in found}) == 6
    assert sc.detect(oracle, c, maps, sc.gray_pair(sc.two_colour_scene(synth, c, 1)[0])[0])["counts"] == [0, 0]


def test_every_frame_is_the_single_frame_call(pkg, world):
    objs, counts, means, npix, disp = world["batch"]
    c = world["c"]
    for f in range(len(ORDER)):
        m, rect, det = fresh(pkg, c, world["maps"])
        got = pkg.estimate_frame_classes(m, rect, det, world["lefts"][f], world["rights"][f], c["Q"], world["ranges"], min_area=sc.MIN_AREA,
                                         max_objects=CAP, want_disp=True)
        close(det, m, rect)
        assert objs[f] == got[0], f
        assert counts[f].tolist() == [sum(o[4] == k for o in got[0]) for k in (0, 1)], f
        assert np.array_equal(npix[f], got[2]), f
        np.testing.assert_allclose(means[f], got[1], rtol=1e-9, atol=0)
        if f == GRAY:
            assert objs[f] == [] and counts[f].tolist() == [0, 0] and len(means[f]) == 0
            assert (disp[f] == DISP0).all()                               # the matcher was skipped: the frame is untouched
        else:
            assert min(counts[f]) >= 1 and npix[f].sum() > 0 and np.array_equal(disp[f], got[3]), f
    assert np.array_equal(disp[1], disp[2]) and objs[1] == objs[2] and means[1].tobytes() == means[2].tobytes()
    assert not np.array_equal(disp[0], disp[1])


def test_seed_3_against_the_cpu_chain(oracle, world):
    objs, counts, means, npix, disp = world["batch"]
    f = ORDER.index(3)
    want = sc.oracle_chain(oracle, world["c"], world["maps"], world["lefts"][f], world["rights"][f], CAP)
    assert objs[f] == want[0] and counts[f].tolist() == want[1] == [2, 2]
    assert np.array_equal(disp[f], want[4])
    assert np.array_equal(npix[f], want[3]) and all(npix[f][[o[4] == k for o in objs[f]]].sum() > 0 for k in (0, 1))
    np.testing.assert_allclose(means[f], want[2], rtol=1e-9, atol=0)


def same(a, b, frames_a, frames_b):
    for fa, fb in zip(frames_a, frames_b):
        assert a[0][fa] == b[0][fb] and a[1][fa].tobytes() == b[1][fb].tobytes()
        assert a[2][fa].tobytes() == b[2][fb].tobytes() and a[3][fa].tobytes() == b[3][fb].tobytes()
        assert a[4][fa].tobytes() == b[4][fb].tobytes()


def test_run_to_run_and_a_batch_of_one(world):
    n = len(ORDER)
    again = run_batch(world, world["lefts"], world["rights"])
    same(world["batch"], again, range(n), range(n))
    one = run_batch(world, world["lefts"][:1], world["rights"][:1])
    same(world["batch"], one, [0], [0])
    # ... and a batch that starts elsewhere, so that the chunks pair the frames differently
    tail = run_batch(world, world["lefts"][1:], world["rights"][1:])
    same(world["batch"], tail, range(1, n), range(n - 1))


def test_device_form_is_the_host_form(pkg, world):
    import torch
    c, n = world["c"], len(ORDER)
    rw, rh = c["roi"][2], c["roi"][3]
    d_l, d_r = torch.from_numpy(world["lefts"]).cuda(), torch.from_numpy(world["rights"]).cuda()
    d_obj = torch.full((n, CAP * 32), 0xA5, dtype=torch.uint8, device="cuda")
    d_cnt = torch.full((n, 2), -7, dtype=torch.int32, device="cuda")
    d_mean = torch.full((n, CAP), -777.0, dtype=torch.float64, device="cuda")
    d_npix = torch.full((n, CAP), -777, dtype=torch.int32, device="cuda")
    dbuf = torch.full((n, rh + 1, rw + 3), DISP0, dtype=torch.int16, device="cuda")       # padded rows and frames
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    world["est"].estimate_device(d_l, d_r, c["Q"], world["ranges"], None, d_obj, d_cnt, d_mean, d_npix, d_disp=dbuf[:, :rh, :rw],
                                 min_area=sc.MIN_AREA, stream=s.cuda_stream)
    s.synchronize()
    objs, counts, means, npix, disp = world["batch"]
    cnt, mean, pix, full = d_cnt.cpu().numpy(), d_mean.cpu().numpy(), d_npix.cpu().numpy(), dbuf.cpu().numpy()
    rec = d_obj.cpu().numpy().view(pkg.OBJECT_DTYPE).reshape(n, CAP)
    assert np.array_equal(cnt, counts)
    for f in range(n):
        k = int(cnt[f].sum())
        o = rec[f, :k]
        assert list(zip(o["x"].tolist(), o["y"].tolist(), o["width"].tolist(), o["height"].tolist(), o["cls"].tolist())) == objs[f]
        assert mean[f, :k].tobytes() == means[f].tobytes() and pix[f, :k].tobytes() == npix[f].tobytes()
        assert (mean[f, k:] == -777.0).all() and (pix[f, k:] == -777).all()
        assert rec[f, k:].tobytes() == bytes([0xA5]) * (32 * (CAP - k))
        assert np.array_equal(full[f, :rh, :rw], disp[f])
    assert (full[:, rh:, :] == DISP0).all() and (full[:, :, rw:] == DISP0).all()


def test_single_calls_on_the_borrowed_handles_afterwards(pkg, world):
    c = world["c"]
    left, right = world["lefts"][0], world["rights"][0]
    run_batch(world, world["lefts"], world["rights"])
    got = pkg.estimate_frame(world["m"], world["rect"], world["det"], left, right, c["Q"], min_area=sc.MIN_AREA, want_disp=True)
    m, rect, det = fresh(pkg, c, world["maps"])
    new = pkg.estimate_frame(m, rect, det, left, right, c["Q"], min_area=sc.MIN_AREA, want_disp=True)
    close(det, m, rect)
    assert len(got[0]) >= 1 and got[2].sum() > 0
    for a, b in zip(got, new):
        assert np.array_equal(a, b)


def test_refusals_that_need_the_estimator(pkg, world):
    import ctypes as C
    B = pkg.binding
    L = B.lib()
    c = world["c"]
    W, H = c["W"], c["H"]
    rw, rh = c["roi"][2], c["roi"][3]
    buf = np.zeros(2 * 3 * W * H + 64, np.uint8)
    out = np.zeros(1 << 16, np.uint8)
    q = (C.c_double * 16)(*np.asarray(c["Q"], np.float64).reshape(16))
    rng = (B.HsvRange * 3)(*[B.HsvRange((C.c_int * 3)(0, 150, 0), (C.c_int * 3)(9, 255, 255)) for _ in range(3)])

    def call(n=2, pitch=3 * W, stride=3 * W * H, cls=(0, 1), nr=2, K=2, disp=None, dpitch=2 * rw, dstride=2 * rw * rh):
        return L.rtdm_estimate_batch(world["est"]._h, n, buf.ctypes.data, pitch, stride, buf.ctypes.data, pitch, stride, q, rng,
                                     (C.c_int * 3)(*cls), nr, K, sc.MIN_AREA, 1, 25.0, out.ctypes.data, out.ctypes.data + 32768,
                                     out.ctypes.data + 40000, out.ctypes.data + 50000, disp, dpitch, dstride)

    assert call() == 0 and call(n=0) == 0 and call(n=1, stride=0) == 0
    assert call(cls=(0, 1, 2), nr=3, K=3) == -1                           # more classes than the detector was made for
    assert call(pitch=3 * W - 1) == -2 and call(stride=3 * W * H - 1) == -2
    d = np.zeros(2 * rw * rh + 8, np.int16).ctypes.data
    assert call(disp=d) == 0
    assert call(disp=d, dpitch=2 * rw - 2) == -2 and call(disp=d, dstride=2 * rw * rh - 2) == -2 and call(disp=d, dpitch=2 * rw + 1) == -2
    h = C.c_void_p()
    assert L.rtdm_estimator_create(world["m"]._h, world["rect"]._h, world["det"]._h, 0, 4, C.byref(h)) == -2
    small = pkg.HIPObjectDetector(rw - 1, rh)
    assert L.rtdm_estimator_create(world["m"]._h, world["rect"]._h, small._h, 1, 4, C.byref(h)) == -2 and not h.value
    small.close()
