#!/usr/bin/env python3
"""Random parity soak of StereoSGBM with numDisparities > 256 (the wide-line path pass, k_sgm_wide.hip; run on the GPU box):
random D (272 .. 4080), minDisparity, frame shapes, block sizes, both modes, the library's parameter coercions, device batches
of 1-3 pairs, and one case in four with the wide form forced (rtdm_debug_sgm_wide_paths 1 / 4) -- against
oracle/sgm_oracle.c, tolerance 0.
    python tools/soak_sgm_wide.py [first_seed=700000] [count=120]"""
import importlib, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
pkg = importlib.import_module("rt-depth-map_amd")
from oracle import oracle as orc
orc.build()
first = int(sys.argv[1]) if len(sys.argv) > 1 else 700000
count = int(sys.argv[2]) if len(sys.argv) > 2 else 120
lib = pkg.binding.lib()
st = torch.cuda.current_stream().cuda_stream
bad = 0
for seed in range(first, first + count):
    rng = np.random.default_rng(seed)
    D = int(rng.choice([272, 288, 320, 336, 384, 400, 512, 528, 640, 768, 1008, 1024, 1040, 1536, 2048, 4080]))
    minD = int(rng.choice([0, 0, 7, -13, -D // 2]))
    W = min(D + abs(minD) + int(rng.choice([1, 9, 33, 64, 65, 130, 301])), 4096)
    H = int(rng.integers(3, 40))
    n = int(rng.choice([1, 1, 2, 3]))
    force = int(rng.choice([0, 0, 0, 1, 4]))
    kw = dict(blockSize=int(rng.choice([1, 3, 5, 5, 7, 9, 11, 4, 19])), minDisparity=minD,
              uniquenessRatio=int(rng.choice([10, 0, 25, -1, 100])), speckleWindowSize=int(rng.choice([100, 0, 20])),
              speckleRange=int(rng.choice([32, 1, 2])), disp12MaxDiff=int(rng.choice([1, -1, 2])),
              P1=int(rng.choice([600, 8, 100, 0])), P2=int(rng.choice([2400, 700, 3000, 0, 20000])), paths=int(rng.choice([8, 5])))
    Ls, Rs = pkg.synth.make_stream(seed % 100000, n, W, H, min(D, 256))
    if rng.random() < 0.2:                       # plateaus: many exact ties
        Ls = (Ls // 32 * 32).astype(np.uint8); Rs = (Rs // 32 * 32).astype(np.uint8)
    lib.rtdm_debug_sgm_wide_paths(force)
    try:
        m = pkg.HIPSemiGlobalMatcher(numOfDisparities=D, width=W, height=H, max_batch=n, **kw)
        dL, dR = torch.from_numpy(Ls).cuda(), torch.from_numpy(Rs).cuda()
        dD = torch.empty((n, H, W), dtype=torch.int16, device="cuda")
        try:
            m.compute_device(dL, dR, dD, st)
            torch.cuda.synchronize()
            got, refused = dD.cpu().numpy(), False
        except pkg.binding.RtdmError:
            got, refused = None, True
        variant = m.path_variant
        m.close()
    finally:
        lib.rtdm_debug_sgm_wide_paths(0)
    for i in range(n):
        try:
            want = orc.sgm_compute(Ls[i], Rs[i], numDisparities=D, **kw)
        except ValueError:
            want = None
        if refused:
            if want is not None and n == 1:
                bad += 1; print("REFUSED ONLY BY THE DEVICE seed", seed, W, H, D, kw)
            break
        if want is None or not np.array_equal(got[i], want):
            bad += 1
            print("MISMATCH seed", seed, "frame", i, W, H, D, force, variant, kw,
                  "pixels", -1 if want is None else int((got[i] != want).sum()), flush=True)
    if (seed - first) % 20 == 0:
        print("case", seed - first, "D", D, "W", W, "variant", variant, "mismatches so far", bad, flush=True)
print("SOAK_SGM_WIDE cases", count, "mismatches", bad)
