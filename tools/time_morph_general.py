#!/usr/bin/env python3
"""Time of rtdm_morph_run_device, 16 device-resident frames of 1280x720 per call, HIP events on the torch stream (run on the
GPU box):
    python3 tools/time_morph_general.py [reps=20] [rounds=5]
Rows: the fused 10x10 kernel (k_morph_open_close, the default route), the general path (k_morph_pass of k_morph_general.hip)
at the same setting through rtdm_debug_morph_general, and the general path's ERODE alone with ELLIPSE 3x3, 10x10, 31x31 and
63x63.  Per row: the median and the range over `rounds` timings of `reps` calls each, in us per frame, the number of
launches, and the algorithmic HBM bytes per pixel (one read and one write per launch)."""
import importlib, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
pkg = importlib.import_module("rt-depth-map_amd")

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
W, H, n = 1280, 720, 16
E = pkg.MORPH_ELLIPSE
# (label, force the general path, op, element, launches)
ROWS = [("fused k_morph_open_close, OPEN_CLOSE ELLIPSE 10x10", 0, pkg.MORPH_OPEN_CLOSE, (E, (10, 10)), 1),
        ("general, OPEN_CLOSE ELLIPSE 10x10", 1, pkg.MORPH_OPEN_CLOSE, (E, (10, 10)), 4),
        ("general, ERODE ELLIPSE 3x3", 0, pkg.MORPH_ERODE, (E, (3, 3)), 1),
        ("general, ERODE ELLIPSE 10x10", 0, pkg.MORPH_ERODE, (E, (10, 10)), 1),
        ("general, ERODE ELLIPSE 31x31", 0, pkg.MORPH_ERODE, (E, (31, 31)), 1),
        ("general, ERODE ELLIPSE 63x63", 0, pkg.MORPH_ERODE, (E, (63, 63)), 1)]

rng = np.random.default_rng(1)
frames = rng.integers(0, 256, (n, H, W), dtype=np.uint8)
frames[:, 100:300, 200:700] = 255
d_in = torch.from_numpy(frames).cuda(); d_out = torch.empty_like(d_in)
st = torch.cuda.current_stream()
lib = pkg.binding.lib()
mf = pkg.HIPMorphologicalFilter(W, H, 8, max_batch=n)
out, sums = [], {}
for label, force, op, element, launches in ROWS:
    mf.set_op(op, element)
    lib.rtdm_debug_morph_general(force)
    try:
        for _ in range(3):
            mf.run_device(d_in, d_out, st.cuda_stream)
        torch.cuda.synchronize()
        us = []
        for _ in range(rounds):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(st)
            for _ in range(reps):
                mf.run_device(d_in, d_out, st.cuda_stream)
            b.record(st); b.synchronize()
            us.append(a.elapsed_time(b) * 1e3 / reps / n)
    finally:
        lib.rtdm_debug_morph_general(0)
    sums[label] = int(d_out.sum(dtype=torch.int64).item())
    row = dict(row=label, launches=launches, us_per_frame_median=round(statistics.median(us), 2),
               us_per_frame_range=[round(min(us), 2), round(max(us), 2)], algorithmic_bytes_per_pixel=2 * launches,
               GBps_algorithmic=round(2 * launches * W * H / statistics.median(us) / 1e3, 1), checksum=sums[label])
    out.append(row)
    print(json.dumps(row), flush=True)
mf.close()
assert sums[ROWS[0][0]] == sums[ROWS[1][0]], "the two routes of the default setting disagree"
print(json.dumps(dict(general_over_fused_at_default=round(out[1]["us_per_frame_median"] / out[0]["us_per_frame_median"], 2),
                      frames_per_call=n, width=W, height=H, reps=reps, rounds=rounds)))
