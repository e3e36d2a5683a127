#!/usr/bin/env python3
"""Time of rtdm_sgm_compute_device with the wide-line path pass (k_sgm_wide.hip), 1280x720 synthetic pairs, HIP events on the
torch stream (run on the GPU box):
    python3 tools/time_sgm_wide.py [reps=5]
Rows: numDisparities 256 (the narrow kernels, reference point), 272, 384, 512, 1024; MODE_SGBM (5 paths) and MODE_HH (8);
1 and 8 pairs per call; ms per pair for the whole call.  D = 256 also runs forced onto the wide pass (rtdm_debug_sgm_wide_paths)
in both forms.  Parity: frame 0 of one call per D against oracle/sgm_oracle.c (MODE_SGBM, tolerance 0)."""
import importlib, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
pkg = importlib.import_module("rt-depth-map_amd")
from oracle import oracle as orc

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
W, H = 1280, 720
lib = pkg.binding.lib()
st = torch.cuda.current_stream()
ROWS = [(256, 0), (256, 1), (256, 4), (272, 0), (384, 0), (512, 0), (512, 4), (1024, 0), (1024, 4)]
parity = {}
for D, force in ROWS:
    for paths in (5, 8):
        for n in (1, 8):
            dL = torch.empty((n, H, W), dtype=torch.uint8, device="cuda"); dR = torch.empty_like(dL)
            dD = torch.empty((n, H, W), dtype=torch.int16, device="cuda")
            pkg.synth_pairs_device(dL, dR, 0, 200)
            lib.rtdm_debug_sgm_wide_paths(force)
            try:
                m = pkg.HIPSemiGlobalMatcher(numOfDisparities=D, width=W, height=H, max_batch=n, paths=paths)
                m.compute_device(dL, dR, dD, st.cuda_stream); torch.cuda.synchronize()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(st)
                for _ in range(reps):
                    m.compute_device(dL, dR, dD, st.cuda_stream)
                b.record(st); b.synchronize()
                ms = a.elapsed_time(b) / reps / n
                variant = m.path_variant
                m.close()
            finally:
                lib.rtdm_debug_sgm_wide_paths(0)
            if paths == 5 and n == 1 and force == 0 and D in (272, 512):
                L, R = dL[0].cpu().numpy(), dR[0].cpu().numpy()
                parity[D] = bool(np.array_equal(dD[0].cpu().numpy(), orc.sgm_compute(L, R, numDisparities=D, paths=5)))
            row = dict(D=D, forced=force, paths=paths, pairs_per_call=n, variant=variant, ms_per_pair=round(ms, 3),
                       domain_columns=W - D)
            print(json.dumps(row), flush=True)
            del dL, dR, dD
            torch.cuda.empty_cache()
print(json.dumps({"parity_frame0_mode_sgbm": parity}))
