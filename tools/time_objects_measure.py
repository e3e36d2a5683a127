#!/usr/bin/env python3
"""Time of the per-object measurements (rtdm_objects_measure_device, rtdm_estimate_batch_measured) on
the GPU box, one JSON line per row:
    python3 tools/time_objects_measure.py call [reps=20] [rounds=7]
        rtdm_objects_measure_device on the lists, label planes and masks of 16 frames at 934x404 (the frames of
        tools/time_objects_labels.py), nquant in {0, 1, 3, 8}, both disparity modes, both plane forms, next to
        rtdm_depth_objects_labels_device on the same lists.
    python3 tools/time_objects_measure.py extremes [reps=20] [rounds=7]
        dots-257x131 (8320 one-pixel objects) and one blob that fills 934x404, nquant 0 and 8, both modes.
    python3 tools/time_objects_measure.py estimator [tree] [reps=6] [rounds=7]
        rtdm_estimate_batch with n in {1, 4, 16} host frame pairs per call (the set-up of tools/time_estimate_batch.py), and --
        where the tree has it -- rtdm_estimate_batch_measured on the same handles, alternating; and rtdm_xyz_map on one 934x404
        map.  `tree`: the checkout whose package is loaded (default: this one), so that the same command times a built parent.
    python3 tools/time_objects_measure.py all PARENT_TREE OUT [times=7]
        call and extremes once; estimator and `bench.py --gpus 1 --steps 20 --warmup 3` `times` times for PARENT_TREE and this
        tree in turn, each in a fresh process.  Writes OUT: the rows, and the gates -- this tree's median against the parent's
        medians of the same visit.
HIP events on the torch stream around `reps` calls (the estimator and rtdm_xyz_map, which synchronise: host clock); per row the
median and the range over `rounds` timings after 3 warm-up calls."""
import importlib, json, os, statistics, subprocess, sys, time
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
mode = sys.argv[1] if len(sys.argv) > 1 else ""
args = sys.argv[2:]

W, H = 934, 404
COLOURS = [(200, 20, 20), (200, 200, 20), (20, 200, 20), (20, 200, 200), (20, 20, 200)]
RANGES = [((0, 150, 0), (9, 255, 255))] + [((h - 8, 150, 0), (h + 8, 255, 255)) for h in (30, 60, 90, 120)]


def stats(us):
    return dict(median=round(statistics.median(us), 2), range=[round(min(us), 2), round(max(us), 2)])


if mode == "all":
    parent, out = os.path.abspath(args[0]), args[1]
    times = int(args[2]) if len(args) > 2 else 7
    rows = []

    def child(script, *a, cwd=None):
        r = subprocess.run([sys.executable, script] + list(a), capture_output=True, text=True, timeout=400, cwd=cwd)
        if r.returncode != 0:
            raise SystemExit("%s %s failed (%d):\n%s" % (script, " ".join(a), r.returncode, r.stderr[-2000:]))
        return [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]

    me = os.path.abspath(__file__)
    for m in ("call", "extremes"):
        rows.extend(child(me, m))
    gate = {"parent": {}, "this": {}}
    for _ in range(times):                                  # parent and child in turn, one visit
        for who, tree in (("parent", parent), ("this", HERE)):
            for row in child(me, "estimator", tree):
                row["tree"] = who
                rows.append(row)
                for key in ("batch_us_per_frame", "xyz_map_us"):
                    if key in row:
                        gate[who].setdefault((row["row"], row.get("n", 0)), []).append(row[key]["median"])
            for row in child(os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "3", cwd=tree):
                if "value" in row:
                    rows.append(dict(row="bench.py --gpus 1 --steps 20 --warmup 3", tree=who, value=row["value"], unit=row["unit"],
                                     ms_per_step=row["ms_per_step"]))
                    gate[who].setdefault(("bench.py headline", 0), []).append(row["value"])
    verdicts = []
    for key in gate["parent"]:
        p, c = gate["parent"][key], gate["this"][key]
        verdicts.append(dict(row="gate: " + key[0], n=key[1], parent=p, this=c, parent_spread=round(max(p) - min(p), 2),
                             this_median_minus_parent_median=round(statistics.median(c) - statistics.median(p), 2),
                             within_parent_spread=bool(abs(statistics.median(c) - statistics.median(p)) <= max(p) - min(p))))
    with open(out, "w") as f:
        for row in rows + verdicts:
            f.write(json.dumps(row) + "\n")
    print("\n".join(json.dumps(v) for v in verdicts))
    raise SystemExit(0)

tree = HERE
if mode == "estimator" and args and not args[0].isdigit():
    tree = os.path.abspath(args.pop(0))
reps = int(args[0]) if args else (6 if mode == "estimator" else 20)
rounds = int(args[1]) if len(args) > 1 else 7
sys.path.insert(0, tree)
import numpy as np
import torch
pkg = importlib.import_module("rt-depth-map_amd")
assert torch.cuda.is_available(), "no GPU: nothing is timed"
st = torch.cuda.current_stream()
Q = np.array([[1, 0, 0, -467], [0, 1, 0, -202], [0, 0, 0, 900], [0, 0, 1 / 60.0, 0]], np.float64)


def scene(seed, W=W, H=H):
    rng = np.random.default_rng(seed)
    g = rng.integers(60, 200, (H, W), dtype=np.uint8)
    rgb = np.stack([g, g, g], -1)
    yy, xx = np.mgrid[0:H, 0:W]
    for k in range(15):
        cx, cy, a, b = rng.integers(40, W - 40), rng.integers(30, H - 30), rng.integers(12, 70), rng.integers(10, 50)
        rgb[((xx - cx) / a) ** 2 + ((yy - cy) / b) ** 2 <= 1] = COLOURS[k % 5]
    for _ in range(40):
        x, y = rng.integers(0, W - 3), rng.integers(0, H - 3)
        rgb[y:y + 3, x:x + 3] = COLOURS[int(rng.integers(0, 5))]
    return np.ascontiguousarray(rgb)


def timed(call, per):
    """median and range of the time of one call, divided by `per`, in microseconds"""
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    us = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(st)
        for _ in range(reps):
            call()
        b.record(st); b.synchronize()
        us.append(a.elapsed_time(b) * 1e3 / reps / per)
    return stats(us)


def detect(frames, K, cap, identity=False, min_area=100):
    """the detector's device lists, label planes and masks of the frames"""
    n, Hf, Wf, _ = frames.shape
    det = pkg.HIPObjectDetector(Wf, Hf, max_batch=n, max_classes=K)
    if identity:
        det.set_op(pkg.MORPH_ERODE, (pkg.MORPH_RECT, (1, 1)))
    o = dict(obj=torch.zeros((n, cap * 32), dtype=torch.uint8, device="cuda"), cnt=torch.zeros((n, K), dtype=torch.int32, device="cuda"),
             roi=torch.zeros((n, 4), dtype=torch.int32, device="cuda"), lab=torch.zeros((n, K, Hf, Wf), dtype=torch.int32, device="cuda"),
             masks=torch.zeros((n, K, Hf, Wf), dtype=torch.uint8, device="cuda"))
    det.detect_labels_device(torch.from_numpy(frames).cuda(), RANGES[:K], None, o["obj"], o["cnt"], o["roi"], d_masks=o["masks"], d_labels=o["lab"],
                             min_area=min_area, capacity=cap, stream=st.cuda_stream)
    torch.cuda.synchronize()
    det.close()
    return o


def random_maps(n, Hf, Wf):
    rng = np.random.default_rng(4)
    disp = rng.integers(32, 1024, (n, Hf, Wf)).astype(np.int16)
    disp[rng.random((n, Hf, Wf)) < 0.2] = -16
    return torch.from_numpy(disp).cuda()


def measure_rows(title, o, d_disp, n, K, cap, quants, extra):
    Hf = d_disp.shape[1]
    d_meas = torch.zeros((n, cap * 88), dtype=torch.uint8, device="cuda")
    ws = torch.empty(pkg.objects_measure_workspace_bytes(n, cap, Hf, 8), dtype=torch.uint8, device="cuda")
    for labels, planes in ((True, o["lab"]), (False, o["masks"])):
        for mode_name, dm in (("ROUNDED", pkg.XYZ_ROUNDED), ("FIXED16", pkg.XYZ_FIXED16)):
            row = dict(row=title, planes="labels" if labels else "masks", disparity_mode=mode_name, n=n, classes=K, capacity=cap, reps=reps,
                       rounds=rounds, **extra)
            for nq in quants:
                P = pkg.MeasureParams(disparity_mode=dm, permille=(500, 250, 750, 0, 1000, 100, 900, 990)[:nq])
                row["nquant_%d_us_per_frame" % nq] = timed(lambda: pkg.objects_measure_device(d_disp, Q, planes, o["obj"], o["cnt"], d_meas, params=P,
                                                                                               labels=labels, capacity=cap, d_workspace=ws,
                                                                                               stream=st.cuda_stream), n)
            torch.cuda.synchronize()
            rec = d_meas.cpu().numpy().view(pkg.MEASURE_DTYPE).reshape(n, cap)
            stored = [min(int(c), cap) for c in o["cnt"].sum(dim=1).tolist()]
            row["pixels_measured"] = int(sum(int(rec[f]["npix"][:stored[f]].sum()) for f in range(n)))
            print(json.dumps(row), flush=True)


if mode == "call":
    n, K, cap = 16, 2, 256
    o = detect(np.stack([scene(10 + i) for i in range(n)]), K, cap)
    d_disp = random_maps(n, H, W)
    d_mean = torch.zeros((n, cap), dtype=torch.float64, device="cuda"); d_npix = torch.zeros((n, cap), dtype=torch.int32, device="cuda")
    ws = torch.empty(pkg.depth_objects_workspace_bytes(n, cap, H), dtype=torch.uint8, device="cuda")
    t = timed(lambda: pkg.depth_objects_labels_device(d_disp, Q, o["lab"], o["obj"], o["cnt"], d_mean, d_npix, capacity=cap, d_workspace=ws,
                                                      stream=st.cuda_stream), n)
    extra = dict(objects_per_frame=round(float(o["cnt"].sum().item()) / n, 1), depth_objects_labels_us_per_frame=t)
    measure_rows("rtdm_objects_measure_device next to rtdm_depth_objects_labels_device", o, d_disp, n, K, cap, (0, 1, 3, 8), extra)
elif mode == "extremes":
    red = np.array(COLOURS[0], np.uint8)
    dots = np.zeros((131, 257), bool); dots[1::2, 1::2] = True
    for name, mask in (("dots-257x131", dots), ("blob-934x404", np.ones((H, W), bool))):
        rgb = np.full(mask.shape + (3,), 128, np.uint8)
        rgb[mask] = red
        cap = 16384 if name.startswith("dots") else 16
        o = detect(rgb[None], 1, cap, identity=True, min_area=1)
        d_disp = random_maps(1, *mask.shape)
        measure_rows("rtdm_objects_measure_device, extremes", o, d_disp, 1, 1, cap, (0, 8), dict(case=name, objects=int(o["cnt"].sum().item())))
elif mode == "estimator":
    sys.path.insert(0, os.path.join(tree, "tests"))
    from oracle import oracle as orc
    import rectify_util as ru
    D, BLOCK, MIN_AREA, CAP, NMAX = 64, 9, 100, 64, 16
    TWO = [((0, 150, 0), (9, 255, 255)), ((110, 150, 0), (130, 255, 255))]

    def pair(c, seed):
        left, right = ru.red_scene(pkg.synth, seed, c["W"], c["H"], D)
        for img in (left, right):                             # the objects of the right half turn blue
            half = img[:, c["W"] // 2:]
            red = half[..., 0] > half[..., 1]
            half[red] = half[red][:, ::-1]
        return left, right

    def clocked(fn, frames):
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        return (time.perf_counter() - t0) * 1e6 / reps / frames

    orc.build()
    c, maps = ru.maps(orc, "1280x720")
    rw, rh = c["roi"][2], c["roi"][3]
    pairs = [pair(c, s) for s in range(1, NMAX + 1)]
    lefts = np.stack([p[0] for p in pairs]); rights = np.stack([p[1] for p in pairs])
    has = hasattr(pkg, "MeasureParams")
    disp = None
    for n in (1, 4, 16):
        rect = pkg.HIPRectifier(*maps, roi=c["roi"], max_batch=n)
        m = pkg.HIPMatcher(numOfDisparities=D, blockSize=BLOCK, width=rw, height=rh, max_batch=n)
        det = pkg.HIPObjectDetector(rw, rh, max_batch=n, max_classes=2)
        est = pkg.HIPEstimator(m, rect, det, max_batch=n, capacity=CAP)
        batch = lambda: est.estimate(lefts[:n], rights[:n], c["Q"], TWO, min_area=MIN_AREA, want_disp=True)                    # noqa: E731
        calls = [("batch_us_per_frame", batch)]
        if has:
            P = pkg.MeasureParams()
            calls.append(("measured_us_per_frame", lambda: est.estimate(lefts[:n], rights[:n], c["Q"], TWO, min_area=MIN_AREA, want_disp=True, measure=P)))
        for _ in range(2):
            got = [fn() for _, fn in calls]
        t = {k: [] for k, _ in calls}
        for _ in range(rounds):
            for k, fn in calls:
                t[k].append(clocked(fn, n))
        row = dict(row="rtdm_estimate_batch", n=n, crop=[rw, rh], reps=reps, rounds=rounds, objects_per_frame=round(float(got[0][1][:n].sum()) / n, 2))
        for k in t:
            row[k] = stats(t[k])
        if has:
            row["measured_over_batch"] = round(row["measured_us_per_frame"]["median"] / row["batch_us_per_frame"]["median"], 3)
        print(json.dumps(row), flush=True)
        disp = got[0][4][0]
        est.close(); det.close(); m.close(); rect.close()
    rp = pkg.HIPReprojector(c["Q"], rw, rh)
    reps = 50
    rp.reprojectImageTo3D(disp)
    t = [clocked(lambda: rp.reprojectImageTo3D(disp), 1) for _ in range(rounds)]
    print(json.dumps(dict(row="rtdm_xyz_map", crop=[rw, rh], reps=reps, rounds=rounds, xyz_map_us=stats(t))), flush=True)
    rp.close()
else:
    raise SystemExit(__doc__)
