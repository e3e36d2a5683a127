#!/usr/bin/env python3
"""Time of rtdm_sgm_compute_device_cn, gray against colour, 1280x720 synthetic pairs, D = 128, HIP events on the torch stream
(run on the GPU box):
    python3 tools/time_sgm_cn.py [pairs_per_call=16] [reps=5]
Rows: MODE_SGBM (5 paths) and MODE_HH (8), gray and colour, preFilterCap 15 and 63; ms per pair for the whole call.  The colour
frames are the gray ones with two derived channels (so the search has the same texture).  Parity: frame 0 of every row against
tests/sgm_cn_ref.py (tolerance 0)."""
import importlib, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
pkg = importlib.import_module("rt-depth-map_amd")
import sgm_cn_ref as ref

n = int(sys.argv[1]) if len(sys.argv) > 1 else 16
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
W, H, D = 1280, 720, 128
st = torch.cuda.current_stream()
gL = torch.empty((n, H, W), dtype=torch.uint8, device="cuda"); gR = torch.empty_like(gL)
pkg.synth_pairs_device(gL, gR, 0, D)
def colour(g):
    g16 = g.to(torch.int16)
    return torch.stack([g, (255 - g16).to(torch.uint8), ((g16 * 3 + 17) % 256).to(torch.uint8)], dim=3).contiguous()
cL, cR = colour(gL), colour(gR)
dD = torch.empty((n, H, W), dtype=torch.int16, device="cuda")
for paths in (5, 8):
    for cap in (15, 63):
        for name, L, R in (("gray", gL, gR), ("colour", cL, cR)):
            m = pkg.HIPSemiGlobalMatcher(numOfDisparities=D, width=W, height=H, max_batch=n, paths=paths, preFilterCap=cap)
            m.compute_device(L, R, dD, st.cuda_stream); torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(st)
            for _ in range(reps):
                m.compute_device(L, R, dD, st.cuda_stream)
            b.record(st); b.synchronize()
            ms = a.elapsed_time(b) / reps / n
            m.close()
            want = ref.sgm_compute_cn(L[0].cpu().numpy(), R[0].cpu().numpy(), preFilterCap=cap, numDisparities=D, paths=paths)
            exact = bool(np.array_equal(dD[0].cpu().numpy(), want))
            print(json.dumps(dict(paths=paths, preFilterCap=cap, frames=name, pairs_per_call=n, ms_per_pair=round(ms, 4),
                                  exact_frame0=exact)), flush=True)
