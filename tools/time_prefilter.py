#!/usr/bin/env python3
"""Time of the prefilter stage alone: the x-Sobel strip kernel (k_prefilter16) against the normalised-response kernel
(k_prefilter_norm.hip) on the same device-resident batch, 32 synthetic 1280x720 pairs, the library's stage events
(rtdm_bm_get_stage_time), run on the GPU box:
    python3 tools/time_prefilter.py [reps=20] [W=1280] [H=720] [n=32]
Per row: ms per launch (one launch filters the n left and the n right frames), ns per pixel, the HBM traffic the kernel
moves by construction (1 byte read + 1 byte written per pixel; the x-Sobel launch also carries the frame fill) as GB/s, and
the ratio to the x-Sobel row.  The stage events of the normalised-response rows also cover the frame fill, which is a launch
of its own there."""
import importlib, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
pkg = importlib.import_module("rt-depth-map_amd")

arg = [int(a) for a in sys.argv[1:]]
reps, W, H, n = (arg + [20, 1280, 720, 32][len(arg):])[:4]
D, w = 64, 9
ROWS = [("xsobel", pkg.PREFILTER_XSOBEL, 9)] + [("norm ws=%d" % ws, pkg.PREFILTER_NORMALIZED_RESPONSE, ws)
                                                 for ws in (5, 9, 21, 63, 89, 91)]

st = torch.cuda.current_stream()
dL = torch.empty((n, H, W), dtype=torch.uint8, device="cuda"); dR = torch.empty_like(dL)
dD = torch.empty((n, H, W), dtype=torch.int16, device="cuda")
pkg.synth_pairs_device(dL, dR, 0, D)
m = pkg.HIPMatcher(numOfDisparities=D, blockSize=w, width=W, height=H, max_batch=n)
base = None
for label, ptype, ws in ROWS:
    m.setPreFilterSize(ws); m.setPreFilterType(ptype)
    m.set_profiling(False)
    for _ in range(3):                                         # warm (and let the strip tuner settle: it times searches only)
        m.compute_device(dL, dR, dD, st.cuda_stream)
    torch.cuda.synchronize()
    m.set_profiling(True); m.reset_stage_times()
    for _ in range(reps):
        m.compute_device(dL, dR, dD, st.cuda_stream)
    torch.cuda.synchronize()
    s = m.stage_times()["prefilter"]
    ms = s["total_ms"] / s["launches"]
    px = 2 * n * W * H
    if base is None:
        base = ms
    print(json.dumps(dict(row=label, preFilterSize=ws, ms_per_launch=round(ms, 4), ns_per_pixel=round(ms * 1e6 / px, 4),
                          bytes_per_pixel=2, implied_GBps=round(2 * px / (ms * 1e-3) / 1e9, 1),
                          ratio_to_xsobel=round(ms / base, 3))), flush=True)
m.close()
