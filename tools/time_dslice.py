#!/usr/bin/env python3
"""Time of rtdm_bm_compute_device with the disparity-sliced search kernel (k_search_dslice in k_search_generic.hip) against
the generic kernel, 1280x720, batches of 8 synthetic pairs, HIP events on the torch stream (run on the GPU box):
    python3 tools/time_dslice.py [reps=10]
Per row: ms per pair for the whole call and for the search stage alone (the library's stage events, a separate run), both
divided by numDisparities, and the search divided by the searched column-disparities (W - D + 1 columns at minD = 0: the
number of searched columns shrinks as D grows, so per-disparity time alone understates large D).
The forced rows go through rtdm_debug_disparity_slice (dt > 0; 0 = the library's choice)."""
import importlib, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
pkg = importlib.import_module("rt-depth-map_amd")

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
W, H, n = 1280, 720, 8
# (label, D, w, cap, forced slice width)
ROWS = [("generic D256 w25 cap63", 256, 25, 63, 0),
        ("dslice D256 w25 cap63 (forced, widest DT that fits)", 256, 25, 63, 4096),
        ("dslice D512 w25 cap63", 512, 25, 63, 0),
        ("dslice D1024 w25 cap63", 1024, 25, 63, 0),
        ("dslice D512 w13 cap31", 512, 13, 31, 0),
        ("dslice D1024 w13 cap31", 1024, 13, 31, 0)]
# slice widths at D = 512, w = 25, cap 63 (4096: capped to the widest that fits LDS, 96 here)
ROWS += [("dslice D512 w25 cap63 dt=%d" % dt, 512, 25, 63, dt) for dt in (16, 32, 48, 64, 4096)]

st = torch.cuda.current_stream()
lib = pkg.binding.lib()
dL = torch.empty((n, H, W), dtype=torch.uint8, device="cuda"); dR = torch.empty_like(dL)
dD = torch.empty((n, H, W), dtype=torch.int16, device="cuda")
out = []
for label, D, w, cap, dt in ROWS:
    pkg.synth_pairs_device(dL, dR, 0, min(D, 256))
    lib.rtdm_debug_disparity_slice(dt)
    try:
        m = pkg.HIPMatcher(numOfDisparities=D, blockSize=w, preFilterCap=cap, width=W, height=H, max_batch=n)
        m.compute_device(dL, dR, dD, st.cuda_stream); torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(st)
        for _ in range(reps):
            m.compute_device(dL, dR, dD, st.cuda_stream)
        b.record(st); b.synchronize()
        call_ms = a.elapsed_time(b) / reps / n
        m.set_profiling(True); m.reset_stage_times()
        for _ in range(reps):
            m.compute_device(dL, dR, dD, st.cuda_stream)
        torch.cuda.synchronize()
        s = m.stage_times()["search"]
        search_ms = s["total_ms"] / s["frames"]
        variant = m.search_variant
        m.close()
    finally:
        lib.rtdm_debug_disparity_slice(0)
    row = dict(row=label, D=D, w=w, cap=cap, forced_dt=dt, variant=variant, ms_per_pair=round(call_ms, 4),
               us_per_pair_per_disparity=round(call_ms * 1e3 / D, 3), search_ms_per_pair=round(search_ms, 4),
               search_us_per_pair_per_disparity=round(search_ms * 1e3 / D, 3),
               search_ns_per_pair_per_column_disparity=round(search_ms * 1e6 / (D * (W - D + 1)), 3))
    out.append(row)
    print(json.dumps(row), flush=True)
def pick(label, key):
    return next(r for r in out if r["row"] == label)[key]
g256, d512 = "generic D256 w25 cap63", "dslice D512 w25 cap63"
print(json.dumps({"ratio_D512_dslice_over_D256_generic_search_per_disparity":
                      round(pick(d512, "search_us_per_pair_per_disparity") / pick(g256, "search_us_per_pair_per_disparity"), 3),
                  "ratio_D512_dslice_over_D256_generic_search_per_column_disparity":
                      round(pick(d512, "search_ns_per_pair_per_column_disparity") / pick(g256, "search_ns_per_pair_per_column_disparity"), 3)}))
