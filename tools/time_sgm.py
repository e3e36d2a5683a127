#!/usr/bin/env python3
"""ms per 1280x720 D=128 pair of the StereoSGBM path: MODE_HH (paths 8), MODE_SGBM (5) and MODE_HH4 (4; its default form "vert"
and, in a child process with RTDM_SGM_SWEEP=0, one pass per direction: "half"), `reps` repetitions of ten calls each.  Modes 8
and 5 are checked against the oracle on one frame (SGM_CHECK=0 skips that); the two forms of mode 4 must print the same sha1
(bit-exactness of mode 4 is what tests/test_gpu_sgm_hh4.py pins).  --cost census times the census pixel cost (rtdm_sgm_set_cost,
9 x 7 window) instead of the BT cost; it is not checked here (tests/test_gpu_sgm_census.py pins it), its sha1 is printed.
paths 3 is MODE_SGBM_3WAY: a handle created with paths = 5 and set to the mode (rtdm_sgm_set_mode, the one door to it); it is not
checked here either (tests/test_gpu_sgm_3way.py pins it), its sha1 is printed.
    python tools/time_sgm.py [n=4] [reps=1] [paths=8,5,4] [--cost bt|census]"""
import hashlib, importlib, os, subprocess, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
pkg = importlib.import_module("rt-depth-map_amd")
cost = "bt"
if "--cost" in sys.argv:
    i = sys.argv.index("--cost")
    cost = sys.argv[i + 1]
    del sys.argv[i:i + 2]
    if cost not in ("bt", "census"):
        sys.exit("--cost takes bt or census")
from oracle import oracle as orc
n = int(sys.argv[1]) if len(sys.argv) > 1 else 4
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 1
modes = [int(p) for p in (sys.argv[3] if len(sys.argv) > 3 else "8,5,4").split(",")]
W, H, D = 1280, 720, 128
st = torch.cuda.current_stream().cuda_stream
dL = torch.empty((n, H, W), dtype=torch.uint8, device="cuda"); dR = torch.empty_like(dL)
dD = torch.empty((n, H, W), dtype=torch.int16, device="cuda")
pkg.synth_pairs_device(dL, dR, 0, D)
L, R = dL[n - 1].cpu().numpy(), dR[n - 1].cpu().numpy()
check = os.environ.get("SGM_CHECK", "1") == "1"
for paths in modes:
    sg = pkg.HIPSemiGlobalMatcher(numOfDisparities=D, width=W, height=H, max_batch=n, paths=5 if paths == 3 else paths)
    if paths == 3:
        sg.setMode(sg.MODE_SGBM_3WAY)
    if cost == "census":
        sg.setCost(sg.COST_CENSUS, (9, 7))
    for _ in range(2): sg.compute_device(dL, dR, dD, st)
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(10): sg.compute_device(dL, dR, dD, st)
        torch.cuda.synchronize(); ms.append((time.perf_counter() - t0) / 10 / n * 1e3)
    out = dD[n - 1].cpu().numpy()
    ok = bool(np.array_equal(out, orc.sgm_compute(L, R, numDisparities=D, paths=paths))) if check and paths in (5, 8) and cost == "bt" else None
    print("paths %d %-5s %-6s: %s ms per pair (%d pairs per call) exact=%s sha1=%s" % (
        paths, sg.path_variant, cost, " ".join("%.4f" % m for m in ms), n, ok, hashlib.sha1(out.tobytes()).hexdigest()[:12]), flush=True)
    sg.close()
if 4 in modes and os.environ.get("RTDM_SGM_SWEEP", "1") != "0":
    # RTDM_SGM_SWEEP is read once per process: the "half" form of mode 4 runs in a child (this process holds no work by now)
    torch.cuda.synchronize()
    subprocess.check_call([sys.executable, os.path.abspath(__file__), str(n), str(reps), "4", "--cost", cost], env=dict(os.environ, RTDM_SGM_SWEEP="0"))
