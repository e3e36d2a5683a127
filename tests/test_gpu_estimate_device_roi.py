"""rtdm_estimator_set_device_roi: the batched loop body with the matcher reading every frame's union box
from device memory, against the default mode on handles of equal parameters -- host form and device form, own pixels on and
off, measured and unmeasured, bit for bit in every output including what must stay untouched.  The scenes are those of
tests/estimate_batch_scenes.py (two classes); the batch holds a frame without objects inside, one at the end of a chunk and a
whole chunk of them at its end.  Chunks are 2 frames, so n exceeds every batch."""
import numpy as np
import pytest

import estimate_batch_scenes as sc
import rectify_util as ru
from stream_gate import StreamGate

pytestmark = pytest.mark.gpu

CAP = 16
ORDER = [1, 2, None, 3, 5, None, None, None]     # scene seeds; None: the gray pair without objects
DISP0 = 0x5A5A
ROI1 = (20, 10, 150, 100)                        # what the caller has set on the matcher before


@pytest.fixture(scope="module")
def pkg():
    import torch                         # torch first: it brings its own HIP runtime and must initialise before ours
    assert torch.cuda.is_available()
    from conftest import load
    return load()


def handles(pkg, c, maps, device_roi):
    rw, rh = c["roi"][2], c["roi"][3]
    rect = pkg.HIPRectifier(*maps, roi=c["roi"])
    m = pkg.HIPMatcher(numOfDisparities=sc.D, blockSize=sc.BLOCK, width=rw, height=rh, max_batch=2)
    m.setROI1(ROI1)
    det = pkg.HIPObjectDetector(rw, rh, max_batch=4, max_classes=2)
    est = pkg.HIPEstimator(m, rect, det, max_batch=4, capacity=CAP, device_roi=device_roi)
    assert est.device_roi is device_roi
    return dict(m=m, rect=rect, det=det, est=est)


@pytest.fixture(scope="module")
def world(pkg, oracle, synth):
    c, maps = ru.maps(oracle, "320x240")
    scenes = {s: sc.two_colour_scene(synth, c, s) for s in (1, 2, 3, 5)}
    scenes[None] = sc.gray_pair(scenes[1][0])
    lefts = np.stack([scenes[s][0] for s in ORDER]); rights = np.stack([scenes[s][1] for s in ORDER])
    w = dict(c=c, lefts=lefts, rights=rights, ranges=sc.ranges(oracle), off=handles(pkg, c, maps, False), on=handles(pkg, c, maps, True))
    yield w
    for h in (w["on"], w["off"]):
        for k in ("est", "det", "m", "rect"):
            h[k].close()


def host_form(pkg, world, h, measured):
    c = world["c"]
    disp = np.full((len(ORDER), c["roi"][3], c["roi"][2]), DISP0, np.int16)
    return h["est"].estimate(world["lefts"], world["rights"], c["Q"], world["ranges"], min_area=sc.MIN_AREA, disp=disp,
                             measure=pkg.MeasureParams() if measured else None)


def device_form(pkg, world, h, measured, stream=None, before=None):
    """-> the output tensors, sentinels wherever the call must not write"""
    import torch
    c, n = world["c"], len(ORDER)
    rw, rh = c["roi"][2], c["roi"][3]
    d_l, d_r = torch.from_numpy(world["lefts"]).cuda(), torch.from_numpy(world["rights"]).cuda()
    out = dict(obj=torch.full((n, CAP * 32), 0xA5, dtype=torch.uint8, device="cuda"),
               cnt=torch.full((n, 2), -7, dtype=torch.int32, device="cuda"),
               mean=torch.full((n, CAP), -777.0, dtype=torch.float64, device="cuda"),
               npix=torch.full((n, CAP), -777, dtype=torch.int32, device="cuda"),
               disp=torch.full((n, rh + 1, rw + 3), DISP0, dtype=torch.int16, device="cuda"))
    if measured:
        out["meas"] = torch.full((n, CAP * 88), 0xC3, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    if before:
        before()
    h["est"].estimate_device(d_l, d_r, c["Q"], world["ranges"], None, out["obj"], out["cnt"], out["mean"], out["npix"],
                             d_disp=out["disp"][:, :rh, :rw], min_area=sc.MIN_AREA, stream=stream, d_measures=out.get("meas"),
                             measure=pkg.MeasureParams() if measured else None)
    return out


def same_bytes(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].cpu().numpy().tobytes() == b[k].cpu().numpy().tobytes(), k


@pytest.mark.parametrize("own", [False, True], ids=["class_mask", "own_pixels"])
@pytest.mark.parametrize("measured", [False, True], ids=["plain", "measured"])
def test_both_forms_are_the_default_mode_bit_for_bit(pkg, world, own, measured):
    import torch
    for h in (world["off"], world["on"]):
        h["est"].own_pixels = own
    n = len(ORDER)
    # host form
    a, b = host_form(pkg, world, world["off"], measured), host_form(pkg, world, world["on"], measured)
    objs, counts = a[0], a[1]
    assert [int(cn.sum()) > 0 for cn in counts] == [s is not None for s in ORDER] and counts[:, 0].max() >= 1 and counts[:, 1].max() >= 1
    assert a[0] == b[0] and a[1].tobytes() == b[1].tobytes() and a[4].tobytes() == b[4].tobytes()
    for f in range(n):
        assert a[2][f].tobytes() == b[2][f].tobytes() and a[3][f].tobytes() == b[3][f].tobytes(), f      # mean_cm, npix
        if measured:
            assert a[5][f].tobytes() == b[5][f].tobytes(), f
        assert (a[4][f] == DISP0).all() == (ORDER[f] is None), f          # frames without objects keep what the map held
    assert sum(len(x) for x in objs) >= 8 and sum(int(p.sum()) for p in a[3]) > 0
    # device form
    da, db = device_form(pkg, world, world["off"], measured), device_form(pkg, world, world["on"], measured)
    torch.cuda.synchronize()
    same_bytes(da, db)
    assert np.array_equal(da["cnt"].cpu().numpy(), counts)
    rh, rw = a[4].shape[1:]
    assert np.array_equal(da["disp"].cpu().numpy()[:, :rh, :rw], a[4])
    for h in (world["off"], world["on"]):
        h["est"].own_pixels = False


def test_device_form_never_synchronises(pkg, world):
    import torch
    gate = StreamGate()
    device_form(pkg, world, world["on"], True, stream=gate.stream.cuda_stream)          # warm-up: workspaces, tables, modules
    gate.stream.synchronize()
    got = device_form(pkg, world, world["on"], True, stream=gate.stream.cuda_stream, before=gate.hold)
    gate.event.set()
    gate.stream.synchronize()
    assert gate.released is True
    want = device_form(pkg, world, world["off"], True)
    torch.cuda.synchronize()
    same_bytes(got, want)


def test_the_matchers_roi1_stays_what_the_caller_set(pkg, world, synth):
    c = world["c"]
    rw, rh = c["roi"][2], c["roi"][3]
    host_form(pkg, world, world["on"], False)
    L, R = synth.make_pair(synth.STREAM_SEED + 5, rw, rh, sc.D)
    got = world["on"]["m"].compute(L, R)
    fresh = pkg.HIPMatcher(numOfDisparities=sc.D, blockSize=sc.BLOCK, width=rw, height=rh)
    fresh.setROI1(ROI1)
    want = fresh.compute(L, R)
    fresh.setROI1((0, 0, 0, 0))
    whole = fresh.compute(L, R)
    fresh.close()
    assert np.array_equal(got, want) and not np.array_equal(got, whole)


def test_switching_back_is_the_default_again(pkg, world):
    est = world["on"]["est"]
    est.device_roi = False
    assert est.device_roi is False
    a, b = host_form(pkg, world, world["off"], False), host_form(pkg, world, world["on"], False)
    est.device_roi = True
    assert est.device_roi is True
    assert a[0] == b[0] and a[4].tobytes() == b[4].tobytes()
