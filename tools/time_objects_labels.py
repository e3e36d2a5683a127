#!/usr/bin/env python3
"""Time of the detector's label planes, pixel moments and own-pixel depth at the reference's 934x404 crop (run on the GPU box),
one JSON line per row:
    python3 tools/time_objects_labels.py detect [tree] [reps=20] [rounds=5]
        rtdm_objects_detect_device, n in {1, 4, 16} device-resident frames x K in {1, 2} classes, default filter.  `tree`: the
        checkout whose package is loaded (default: this one), so that the same command times a built copy of the parent.
    python3 tools/time_objects_labels.py labels [reps=20] [rounds=5]
        rtdm_objects_detect_labels_device on the same frames with labels + moments, labels only, and neither.
    python3 tools/time_objects_labels.py depth [reps=20] [rounds=5]
        rtdm_depth_objects_labels_device against rtdm_depth_objects_device on the lists and planes of 16 frames.
    python3 tools/time_objects_labels.py atomics [reps=20] [rounds=5]
        the per-run moment atomics of k_cc_labels: labels + moments against labels only (identity filter) on dots-257x131 (8320
        one-pixel objects), on one blob that fills 934x404 (one run per row) and on 60 % noise at 934x404 (one component of tens
        of thousands of runs: every one of them adds to the same six words).
    python3 tools/time_objects_labels.py all PARENT_TREE OUT [times=7]
        everything above, each in a fresh process; `detect` `times` times for this tree and for PARENT_TREE in turn.  Writes OUT:
        the rows, and per (n, K) the gate -- this tree's median against the parent's medians of the same visit.
HIP events on the torch stream around `reps` calls; per row the median and the range over `rounds` timings after 3 warm-up
calls.  The frames are those of tools/time_objects_batch.py."""
import importlib, json, os, statistics, subprocess, sys
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
mode = sys.argv[1] if len(sys.argv) > 1 else ""
args = sys.argv[2:]

W, H = 934, 404
COLOURS = [(200, 20, 20), (200, 200, 20), (20, 200, 20), (20, 200, 200), (20, 20, 200)]
RANGES = [((0, 150, 0), (9, 255, 255))] + [((h - 8, 150, 0), (h + 8, 255, 255)) for h in (30, 60, 90, 120)]
SHAPES = [(n, K) for n in (1, 4, 16) for K in (1, 2)]


def stats(us):
    return dict(median=round(statistics.median(us), 2), range=[round(min(us), 2), round(max(us), 2)])


if mode == "all":
    parent, out = os.path.abspath(args[0]), args[1]
    times = int(args[2]) if len(args) > 2 else 7
    rows = []

    def child(*a):
        r = subprocess.run([sys.executable, os.path.abspath(__file__)] + list(a), capture_output=True, text=True, timeout=240)
        if r.returncode != 0:
            raise SystemExit("%s failed (%d):\n%s" % (" ".join(a), r.returncode, r.stderr[-2000:]))
        got = [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]
        rows.extend(got)
        return got

    gate = {"this": {s: [] for s in SHAPES}, "parent": {s: [] for s in SHAPES}}
    for _ in range(times):                                  # parent and child in turn, one visit
        for who, tree in (("parent", parent), ("this", HERE)):
            for row in child("detect", tree):
                row["tree"] = who
                gate[who][(row["n"], row["classes"])].append(row["us_per_frame"]["median"])
    for m in ("labels", "depth", "atomics"):
        child(m)
    verdicts = []
    for s in SHAPES:
        p, c = gate["parent"][s], gate["this"][s]
        verdicts.append(dict(row="gate: rtdm_objects_detect_device, this tree against the parent", n=s[0], classes=s[1], parent_us_per_frame=p,
                             this_us_per_frame=c, parent_spread=round(max(p) - min(p), 2),
                             this_median_minus_parent_median=round(statistics.median(c) - statistics.median(p), 2),
                             within_parent_spread=bool(abs(statistics.median(c) - statistics.median(p)) <= max(p) - min(p))))
    with open(out, "w") as f:
        for row in rows + verdicts:
            f.write(json.dumps(row) + "\n")
    print("\n".join(json.dumps(v) for v in verdicts))
    raise SystemExit(0)

tree = HERE
if mode == "detect" and args and not args[0].isdigit():
    tree = os.path.abspath(args.pop(0))
reps = int(args[0]) if args else 20
rounds = int(args[1]) if len(args) > 1 else 5
sys.path.insert(0, tree)
import numpy as np
import torch
pkg = importlib.import_module("rt-depth-map_amd")
assert torch.cuda.is_available(), "no GPU: nothing is timed"
st = torch.cuda.current_stream()


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


def outputs(n, K, cap, Wf=W, Hf=H):
    return dict(obj=torch.zeros((n, cap * 32), dtype=torch.uint8, device="cuda"), cnt=torch.zeros((n, K), dtype=torch.int32, device="cuda"),
                roi=torch.zeros((n, 4), dtype=torch.int32, device="cuda"), lab=torch.zeros((n, K, Hf, Wf), dtype=torch.int32, device="cuda"),
                stats=torch.zeros((n, cap * 48), dtype=torch.uint8, device="cuda"), masks=torch.zeros((n, K, Hf, Wf), dtype=torch.uint8, device="cuda"))


def labels_call(det, d_rgb, K, o, cap, labels, moments, ranges=None, masks=False, min_area=100):
    return lambda: det.detect_labels_device(d_rgb, ranges or RANGES[:K], None, o["obj"], o["cnt"], o["roi"], d_masks=o["masks"] if masks else None,
                                            d_labels=o["lab"] if labels else None, d_stats=o["stats"] if moments else None,
                                            min_area=min_area, capacity=cap, stream=st.cuda_stream)


if mode in ("detect", "labels"):
    frames = np.stack([scene(10 + i) for i in range(16)])
    cap = 256
    for n, K in SHAPES:
        d_rgb = torch.from_numpy(frames[:n]).cuda()
        det = pkg.HIPObjectDetector(W, H, max_batch=n, max_classes=K)
        o = outputs(n, K, cap)
        if mode == "detect":
            t = timed(lambda: det.detect_device(d_rgb, RANGES[:K], None, o["obj"], o["cnt"], o["roi"], capacity=cap, stream=st.cuda_stream), n)
            print(json.dumps(dict(row="rtdm_objects_detect_device", n=n, classes=K, reps=reps, rounds=rounds, us_per_frame=t,
                                  objects_per_frame=round(float(o["cnt"].sum().item()) / n, 1))), flush=True)
        else:
            row = dict(row="rtdm_objects_detect_labels_device", n=n, classes=K, reps=reps, rounds=rounds)
            for name, lab, mom in (("labels_and_moments", True, True), ("labels_only", True, False), ("neither", False, False)):
                row[name + "_us_per_frame"] = timed(labels_call(det, d_rgb, K, o, cap, lab, mom), n)
            row["labels_and_moments_over_neither"] = round(row["labels_and_moments_us_per_frame"]["median"] / row["neither_us_per_frame"]["median"], 3)
            row["objects_per_frame"] = round(float(o["cnt"].sum().item()) / n, 1)
            row["labelled_pixels_per_frame"] = round(float((o["lab"] != 0).sum().item()) / n, 1)
            print(json.dumps(row), flush=True)
        det.close()
elif mode == "depth":
    n, K, cap = 16, 2, 256
    frames = np.stack([scene(10 + i) for i in range(n)])
    d_rgb = torch.from_numpy(frames).cuda()
    det = pkg.HIPObjectDetector(W, H, max_batch=n, max_classes=K)
    o = outputs(n, K, cap)
    labels_call(det, d_rgb, K, o, cap, True, True, masks=True)()
    rng = np.random.default_rng(4)
    disp = rng.integers(32, 1024, (n, H, W)).astype(np.int16)
    disp[rng.random((n, H, W)) < 0.2] = -16
    d_disp = torch.from_numpy(disp).cuda()
    Q = np.array([[1, 0, 0, -467], [0, 1, 0, -202], [0, 0, 0, 900], [0, 0, 1 / 60.0, 0]], np.float64)
    d_mean = torch.zeros((n, cap), dtype=torch.float64, device="cuda"); d_npix = torch.zeros((n, cap), dtype=torch.int32, device="cuda")
    ws = torch.empty(pkg.depth_objects_workspace_bytes(n, cap, H), dtype=torch.uint8, device="cuda")
    row = dict(row="rtdm_depth_objects_labels_device against rtdm_depth_objects_device", n=n, classes=K, capacity=cap, reps=reps, rounds=rounds)
    for name, fn, planes in (("masks", pkg.depth_objects_device, o["masks"]), ("labels", pkg.depth_objects_labels_device, o["lab"])):
        row[name + "_us_per_frame"] = timed(lambda: fn(d_disp, Q, planes, o["obj"], o["cnt"], d_mean, d_npix, capacity=cap, d_workspace=ws,
                                                       stream=st.cuda_stream), n)
        row[name + "_pixels_measured"] = int(d_npix.sum().item())
    row["objects_per_frame"] = round(float(o["cnt"].sum().item()) / n, 1)
    print(json.dumps(row), flush=True)
    det.close()
elif mode == "atomics":
    red = np.array(COLOURS[0], np.uint8)

    def paint(mask):
        rgb = np.full(mask.shape + (3,), 128, np.uint8)
        rgb[mask] = red
        return rgb[None]

    rng = np.random.default_rng(6)
    dots = np.zeros((131, 257), bool); dots[1::2, 1::2] = True
    cases = [("dots-257x131", dots), ("blob-934x404", np.ones((H, W), bool)), ("noise60-934x404", rng.random((H, W)) < 0.6)]
    for name, mask in cases:
        Hf, Wf = mask.shape
        cap = 16384
        det = pkg.HIPObjectDetector(Wf, Hf)
        det.set_op(pkg.MORPH_ERODE, (pkg.MORPH_RECT, (1, 1)))
        d_rgb = torch.from_numpy(paint(mask)).cuda()
        o = outputs(1, 1, cap, Wf, Hf)
        row = dict(row="k_cc_labels: per-run moment atomics", case=name, reps=reps, rounds=rounds)
        for key, mom in (("labels_and_moments", True), ("labels_only", False)):
            row[key + "_us"] = timed(labels_call(det, d_rgb, 1, o, cap, True, mom, min_area=1), 1)
        row["moments_cost_us"] = round(row["labels_and_moments_us"]["median"] - row["labels_only_us"]["median"], 2)
        torch.cuda.synchronize()
        m00 = o["stats"].cpu().numpy().view(pkg.STATS_DTYPE)["m00"][0]
        row["objects"] = int(o["cnt"].sum().item()); row["largest_object_pixels"] = int(m00[:min(row["objects"], cap)].max())
        fg = mask.copy(); fg[0, :] = fg[-1, :] = False; fg[:, 0] = fg[:, -1] = False
        row["runs"] = int((fg[:, 1:] & ~fg[:, :-1]).sum() + fg[:, 0].sum())
        print(json.dumps(row), flush=True)
        det.close()
else:
    raise SystemExit(__doc__)
