#!/usr/bin/env python3
"""Time of the batched loop body at the reference's 1280x720 calibration (crop 934x404, D = 64, blockSize 9, a red and a blue
class; run on the GPU box), one JSON line per row:
    python3 tools/time_estimate_batch.py [reps=6] [rounds=7]
        (a) rtdm_estimate_batch with n in {1, 4, 16} host frame pairs per call (all handles made for n) against a loop of
        rtdm_estimate_frame_classes over the same frames on the same handles, in the same process, host clock (both
        synchronise).  The two ALTERNATE: every round times `reps` batched calls, then `reps` loops.
        (b) rtdm_depth_objects_device on the 16 maps, masks and device lists of those frames (HIP events around `reps` calls,
        workspace made once) against rtdm_depth_stats_device on the same maps: one call per frame and class, host clock (that
        call allocates, synchronises and frees).
Per row: the median and the range over `rounds` timings after 2 warm-up calls, in microseconds per frame.  The frames are
tests/rectify_util.red_scene seeds 1 .. 16 with the objects of the right half turned blue."""
import importlib, json, os, statistics, sys, time
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "tests"))
import numpy as np
import torch
pkg = importlib.import_module("rt-depth-map_amd")
assert torch.cuda.is_available(), "no GPU: nothing is timed"
from oracle import oracle as orc
import rectify_util as ru

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 6
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
D, BLOCK, MIN_AREA, CAP, NMAX = 64, 9, 100, 64, 16
RANGES = [((0, 150, 0), (9, 255, 255)), ((110, 150, 0), (130, 255, 255))]


def stats(us):
    return dict(median=round(statistics.median(us), 2), range=[round(min(us), 2), round(max(us), 2)])


def scene(c, seed):
    left, right = ru.red_scene(pkg.synth, seed, c["W"], c["H"], D)
    for img in (left, right):                             # the objects of the right half turn blue
        half = img[:, c["W"] // 2:]
        red = half[..., 0] > half[..., 1]
        half[red] = half[red][:, ::-1]
    return left, right


def union(objects):
    """The union box of a frame's objects as (x0, y0, x1, y1): frames that share it share a matcher launch."""
    return (min(o[0] for o in objects), min(o[1] for o in objects), max(o[0] + o[2] for o in objects), max(o[1] + o[3] for o in objects))


def timed(fn, frames):
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) * 1e6 / reps / frames


orc.build()
c, maps = ru.maps(orc, "1280x720")
rw, rh = c["roi"][2], c["roi"][3]
pairs = [scene(c, s) for s in range(1, NMAX + 1)]
lefts = np.stack([p[0] for p in pairs]); rights = np.stack([p[1] for p in pairs])
last = None
for n in (1, 4, 16):
    rect = pkg.HIPRectifier(*maps, roi=c["roi"], max_batch=n)
    m = pkg.HIPMatcher(numOfDisparities=D, blockSize=BLOCK, width=rw, height=rh, max_batch=n)
    det = pkg.HIPObjectDetector(rw, rh, max_batch=n, max_classes=2)
    est = pkg.HIPEstimator(m, rect, det, max_batch=n, capacity=CAP)
    batch = lambda: est.estimate(lefts[:n], rights[:n], c["Q"], RANGES, min_area=MIN_AREA, want_disp=True)                    # noqa: E731
    loop = lambda: [pkg.estimate_frame_classes(m, rect, det, lefts[f], rights[f], c["Q"], RANGES, min_area=MIN_AREA, max_objects=CAP,   # noqa: E731
                                               want_disp=True) for f in range(n)]
    for _ in range(2):
        got, want = batch(), loop()
    for f in range(n):
        assert got[0][f] == want[f][0] and np.array_equal(got[3][f], want[f][2]), "the batched call and the loop disagree"
        assert not want[f][0] or np.array_equal(got[4][f], want[f][3]), "the batched call and the loop disagree about a map"
    tb, tl = [], []
    for _ in range(rounds):
        tb.append(timed(batch, n)); tl.append(timed(loop, n))
    ratio = round(statistics.median(tb) / statistics.median(tl), 3)
    print(json.dumps(dict(row="(a) rtdm_estimate_batch against a loop of rtdm_estimate_frame_classes", n=n, frame=[c["W"], c["H"]],
                          crop=[rw, rh], reps=reps, rounds=rounds, objects_per_frame=round(float(got[1][:n].sum()) / n, 2),
                          distinct_rois=len({union(o) for o in got[0] if o}),
                          batch_us_per_frame=stats(tb), loop_us_per_frame=stats(tl), batch_over_loop=ratio)), flush=True)
    if n == NMAX:
        last = got
    est.close(); det.close(); m.close(); rect.close()

# (b) the depth step alone, on what the n = 16 call produced
n = NMAX
objs, counts, _, npix, disp = last
det = pkg.HIPObjectDetector(rw, rh, max_batch=n, max_classes=2)
rect = pkg.HIPRectifier(*maps, roi=c["roi"])
crops = np.stack([rect.rgb(lefts[f]) for f in range(n)])
st = torch.cuda.current_stream()
d_obj = torch.zeros((n, CAP * 32), dtype=torch.uint8, device="cuda")
d_cnt = torch.zeros((n, 2), dtype=torch.int32, device="cuda"); d_roi = torch.zeros((n, 4), dtype=torch.int32, device="cuda")
d_masks = torch.zeros((n, 2, rh, rw), dtype=torch.uint8, device="cuda")
det.detect_device(torch.from_numpy(crops).cuda(), RANGES, None, d_obj, d_cnt, d_roi, d_masks=d_masks, min_area=MIN_AREA, capacity=CAP,
                  stream=st.cuda_stream)
d_disp = torch.from_numpy(disp).cuda()
d_mean = torch.zeros((n, CAP), dtype=torch.float64, device="cuda"); d_npix = torch.zeros((n, CAP), dtype=torch.int32, device="cuda")
ws = pkg.depth_objects_device(d_disp, c["Q"], d_masks, d_obj, d_cnt, d_mean, d_npix, capacity=CAP, stream=st.cuda_stream)
torch.cuda.synchronize()
assert np.array_equal(d_cnt.cpu().numpy(), counts)
for f in range(n):
    assert np.array_equal(d_npix.cpu().numpy()[f, :len(objs[f])], npix[f]), "the kernel alone and the chain disagree"


def old():
    for f in range(n):
        for k in (0, 1):
            boxes = [o[:4] for o in objs[f] if o[4] == k]
            if boxes:
                pkg.depth_stats_device(d_disp[f], c["Q"], d_masks[f, k], boxes)


t_new, t_old = [], []
for _ in range(rounds):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(st)
    for _ in range(reps):
        pkg.depth_objects_device(d_disp, c["Q"], d_masks, d_obj, d_cnt, d_mean, d_npix, capacity=CAP, d_workspace=ws, stream=st.cuda_stream)
    b.record(st); b.synchronize()
    t_new.append(a.elapsed_time(b) * 1e3 / reps / n)
    t_old.append(timed(old, n))
print(json.dumps(dict(row="(b) rtdm_depth_objects_device, 16 frames per call, against rtdm_depth_stats_device per frame and class",
                      crop=[rw, rh], objects_per_frame=round(float(counts.sum()) / n, 2), reps=reps, rounds=rounds,
                      objects_device_us_per_frame=stats(t_new), stats_device_us_per_frame=stats(t_old),
                      ratio_of_medians=round(statistics.median(t_new) / statistics.median(t_old), 3))))
det.close(); rect.close()
