#!/usr/bin/env python3
"""Random parity soak of StereoSGBM with the census pixel cost (run on the GPU box): random census window (all twelve),
numDisparities 16 .. 288, minDisparity, frame shapes, block sizes 1 .. 21, the three modes, the library's parameter coercions,
host calls and device batches of 1-3 pairs, plateau images with many ties, one case in five with rtdm_debug_sgm_cost16 on (it
must change nothing), one in five switching the handle BT -> census first -- against tests/sgm_census_ref.py (N1 and N2 in
NumPy, then the C oracle's stages), tolerance 0.  A frame the reference refuses (block cost + P2 > 32767) must be refused by
the device, and the other way round.
    python tools/soak_sgm_census.py [first_seed=900000] [count=120]"""
import importlib, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
pkg = importlib.import_module("rt-depth-map_amd")
from oracle import oracle as orc
import sgm_census_ref as ref
orc.build()
first = int(sys.argv[1]) if len(sys.argv) > 1 else 900000
count = int(sys.argv[2]) if len(sys.argv) > 2 else 120
lib = pkg.binding.lib()
M = pkg.HIPSemiGlobalMatcher
st = torch.cuda.current_stream().cuda_stream
bad = refused_both = 0
for seed in range(first, first + count):
    rng = np.random.default_rng(seed)
    census = (int(rng.choice([3, 5, 7, 9])), int(rng.choice([3, 5, 7])))
    D = int(rng.choice([16, 32, 48, 64, 96, 128, 160, 256, 272, 288]))
    minD = int(rng.choice([0, 0, 5, -9, -D // 2]))
    W = D + abs(minD) + int(rng.choice([1, 9, 33, 64, 65, 130]))
    H = int(rng.integers(1, 40))
    n = int(rng.choice([1, 1, 2, 3]))
    host = n == 1 and rng.random() < 0.5
    force16 = rng.random() < 0.2
    switch = rng.random() < 0.2
    kw = dict(blockSize=int(rng.choice([1, 3, 5, 5, 7, 9, 11, 4, 13, 21])), minDisparity=minD,
              uniquenessRatio=int(rng.choice([10, 0, 25, -1, 100])), speckleWindowSize=int(rng.choice([100, 0, 20])),
              speckleRange=int(rng.choice([32, 1, 2])), disp12MaxDiff=int(rng.choice([1, -1, 2])),
              P1=int(rng.choice([600, 8, 100, 0])), P2=int(rng.choice([2400, 700, 3000, 0, 20000, 32000])),
              paths=int(rng.choice([8, 5, 4])))
    shift = int(rng.integers(0, max(D // 2, 1)))
    T = rng.integers(0, 256, (n, H, W + shift)).astype(np.float64)
    T = ((T + np.roll(T, 1, 2) + np.roll(T, 1, 1)) / 3).astype(np.uint8)
    if rng.random() < 0.3:                       # plateaus: many exact ties
        T = (T // 32 * 32).astype(np.uint8)
    Ls = np.ascontiguousarray(T[:, :, :W]); Rs = np.ascontiguousarray(T[:, :, shift:shift + W])     # L[x] = R[x - shift]
    if rng.random() < 0.5:                       # unequal exposure: an increasing mapping of the right view
        Rs = (Rs.astype(np.int64) * 3 // 4 + 20).astype(np.uint8)
    lib.rtdm_debug_sgm_cost16(1 if force16 else 0)
    try:
        if switch:
            m = M(numOfDisparities=D, width=W, height=H, max_batch=n, preFilterCap=int(rng.choice([0, 63, 100])), **kw)
            m.setCost(M.COST_CENSUS, census)
        else:
            m = M(numOfDisparities=D, width=W, height=H, max_batch=n, cost=M.COST_CENSUS, census=census, **kw)
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
        except pkg.binding.RtdmError as e:
            if e.status != -6:
                raise
            got, refused = None, True
        m.close()
    finally:
        lib.rtdm_debug_sgm_cost16(0)
    for i in range(n):
        try:
            want = ref.sgm_compute(Ls[i], Rs[i], census=census, numDisparities=D, **kw)
        except ref.CostOverflow:
            want = None
        if refused:
            if want is None:
                refused_both += 1
            elif n == 1:
                bad += 1; print("REFUSED ONLY BY THE DEVICE seed", seed, census, W, H, D, kw, flush=True)
            elif i == n - 1:                     # a refused batch: some frame of it must be refused by the reference
                bad += 1; print("BATCH REFUSED ONLY BY THE DEVICE seed", seed, census, W, H, D, kw, flush=True)
            else:
                continue
            break
        if want is None or not np.array_equal(got[i], want):
            bad += 1
            print("MISMATCH seed", seed, "frame", i, "census", census, W, H, D, "force16", force16, "switch", switch, kw,
                  "pixels", -1 if want is None else int((got[i] != want).sum()), flush=True)
    if (seed - first) % 20 == 0:
        print("case", seed - first, "census", census, "D", D, "W", W, "H", H, "mismatches so far", bad, flush=True)
print("SOAK_SGM_CENSUS cases", count, "mismatches", bad, "refused by both", refused_both)
sys.exit(1 if bad else 0)
