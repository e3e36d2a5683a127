#!/usr/bin/env python3
"""Random parity soak of StereoSGBM with colour frames and preFilterCap (run on the GPU box): random channel count (mostly 3),
preFilterCap 0 .. 127, numDisparities 16 .. 512, minDisparity, frame shapes, block sizes, both modes, the library's parameter
coercions, host calls and device batches of 1-3 pairs, and one case in five with the 16-bit pixel-cost forms forced on gray
(rtdm_debug_sgm_cost16) -- against tests/sgm_cn_ref.py (R1 restated for colour and any ftzero, then the C oracle's stages),
tolerance 0.
    python tools/soak_sgm_cn.py [first_seed=800000] [count=120]"""
import importlib, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
pkg = importlib.import_module("rt-depth-map_amd")
from oracle import oracle as orc
import sgm_cn_ref as ref
orc.build()
first = int(sys.argv[1]) if len(sys.argv) > 1 else 800000
count = int(sys.argv[2]) if len(sys.argv) > 2 else 120
lib = pkg.binding.lib()
st = torch.cuda.current_stream().cuda_stream
bad = refused_both = 0
for seed in range(first, first + count):
    rng = np.random.default_rng(seed)
    cn = int(rng.choice([3, 3, 3, 1]))
    cap = int(rng.choice([0, 5, 15, 16, 31, 47, 63, 64, 95, 96, 97, 110, 127]))
    D = int(rng.choice([16, 32, 48, 64, 96, 128, 160, 256, 272, 384, 512]))
    minD = int(rng.choice([0, 0, 5, -9, -D // 2]))
    W = D + abs(minD) + int(rng.choice([1, 9, 33, 64, 65, 130]))
    H = int(rng.integers(3, 40))
    n = int(rng.choice([1, 1, 2, 3]))
    host = n == 1 and rng.random() < 0.5
    force16 = cn == 1 and rng.random() < 0.2
    kw = dict(blockSize=int(rng.choice([1, 3, 5, 5, 7, 9, 11, 4, 13, 19])), minDisparity=minD,
              uniquenessRatio=int(rng.choice([10, 0, 25, -1, 100])), speckleWindowSize=int(rng.choice([100, 0, 20])),
              speckleRange=int(rng.choice([32, 1, 2])), disp12MaxDiff=int(rng.choice([1, -1, 2])),
              P1=int(rng.choice([600, 8, 100, 0])), P2=int(rng.choice([2400, 700, 3000, 0, 20000])), paths=int(rng.choice([8, 5])))
    shift = int(rng.integers(0, max(D // 2, 1)))
    T = rng.integers(0, 256, (n, H, W + shift, cn)).astype(np.float64)
    T = ((T + np.roll(T, 1, 2) + np.roll(T, 1, 1)) / 3).astype(np.uint8)
    if rng.random() < 0.2:                       # plateaus: many exact ties
        T = (T // 32 * 32).astype(np.uint8)
    Ls = T[:, :, :W]; Rs = T[:, :, shift:shift + W]              # L[x] = R[x - shift]
    if cn == 1:
        Ls, Rs = Ls[..., 0], Rs[..., 0]
    Ls, Rs = np.ascontiguousarray(Ls), np.ascontiguousarray(Rs)
    lib.rtdm_debug_sgm_cost16(1 if force16 else 0)
    try:
        m = pkg.HIPSemiGlobalMatcher(numOfDisparities=D, width=W, height=H, max_batch=n, preFilterCap=cap, **kw)
        try:
            if host:
                got = m.compute(Ls[0], Rs[0])[None]
            else:
                dL, dR = torch.from_numpy(Ls).cuda(), torch.from_numpy(Rs).cuda()
                dD = torch.empty((n, H, W), dtype=torch.int16, device="cuda")
                m.compute_device(dL, dR, dD, st)
                torch.cuda.synchronize()
                got = dD.cpu().numpy()
            refused = False
        except pkg.binding.RtdmError:
            got, refused = None, True
        m.close()
    finally:
        lib.rtdm_debug_sgm_cost16(0)
    for i in range(n):
        try:
            want = ref.sgm_compute_cn(Ls[i], Rs[i], preFilterCap=cap, numDisparities=D, **kw)
        except ref.CostOverflow:
            want = None
        if refused:
            if want is None:
                refused_both += 1
            elif n == 1:
                bad += 1; print("REFUSED ONLY BY THE DEVICE seed", seed, cn, cap, W, H, D, kw, flush=True)
            break
        if want is None or not np.array_equal(got[i], want):
            bad += 1
            print("MISMATCH seed", seed, "frame", i, "cn", cn, "cap", cap, W, H, D, "force16", force16, kw,
                  "pixels", -1 if want is None else int((got[i] != want).sum()), flush=True)
    if (seed - first) % 20 == 0:
        print("case", seed - first, "cn", cn, "cap", cap, "D", D, "W", W, "mismatches so far", bad, flush=True)
print("SOAK_SGM_CN cases", count, "mismatches", bad, "refused by both", refused_both)
