#!/usr/bin/env python3
"""The rows of the StereoSGBM route table ("SGM: routes") that a handle reaches without a test hook, one fresh
handle per row, one pair through `compute` and three through `compute_device`; prints the variant, the sweep count and the
sum of the results.  Meant to run under `rocprofv3 --kernel-trace` on two trees whose dispatch sequences are then compared
(profiles/sgm_plan_launches.txt):
    python tools/sgm_routes_run.py [TREE]          TREE: the checkout whose package is loaded (default: this one)
    python tools/sgm_routes_run.py TREE first      instead: wall time of the first and the second `compute` of a fresh
                                                   MODE_HH handle (1280x720, D = 128) in a process that has run the mode before
    python tools/sgm_routes_run.py TREE cost       instead: the rows of the cost-route table ("SGM: cost routes"), one small call
                                                   pair per case of tests/sgm_cost_routes.py (this checkout's, whatever TREE
                                                   is); compared in profiles/sgm_cost_plan_launches.txt"""
import importlib, os, sys, time
tree = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, tree)
import numpy as np, torch
pkg = importlib.import_module("rt-depth-map_amd")
assert os.path.abspath(pkg.__file__).startswith(tree + os.sep), pkg.__file__

if len(sys.argv) > 2 and sys.argv[2] == "first":
    W, H, D = 1280, 720, 128
    L, R = pkg.synth.make_pair(pkg.synth.STREAM_SEED, W, H, D)
    warm = pkg.HIPSemiGlobalMatcher(numOfDisparities=D, width=W, height=H, paths=8)
    for _ in range(2): warm.compute(L, R)
    warm.close()
    for k in range(3):
        sg = pkg.HIPSemiGlobalMatcher(numOfDisparities=D, width=W, height=H, paths=8)
        t = []
        for _ in range(2):
            t0 = time.perf_counter(); sg.compute(L, R); t.append((time.perf_counter() - t0) * 1e3)
        print("fresh MODE_HH handle %d: first compute %.3f ms, second %.3f ms (%s)" % (k, t[0], t[1], sg.path_variant), flush=True)
        sg.close()
    sys.exit(0)

if len(sys.argv) > 2 and sys.argv[2] == "cost":
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import sgm_cost_routes as routes
    M = pkg.HIPSemiGlobalMatcher
    st = torch.cuda.current_stream().cuda_stream
    for c in routes.CASES:
        frames = c.frames()
        Ls, Rs = np.stack([f[0] for f in frames]), np.stack([f[1] for f in frames])
        pkg.binding.lib().rtdm_debug_sgm_cost16(c.f16)
        sg = M(numOfDisparities=c.D, blockSize=c.bs, P1=routes.P1, P2=c.P2, width=c.W, height=c.H, max_batch=3, preFilterCap=c.cap,
               paths=5 if c.paths == 3 else c.paths, **(dict(cost=M.COST_CENSUS, census=c.census) if c.census else {}))
        if c.paths == 3: sg.setMode(M.MODE_SGBM_3WAY)
        one = sg.compute(Ls[0], Rs[0])
        dD = torch.zeros((3, c.H, c.W), dtype=torch.int16, device="cuda")
        sg.compute_device(torch.from_numpy(Ls).cuda(), torch.from_numpy(Rs).cuda(), dD, st)
        torch.cuda.synchronize()
        print("%s (%s) paths %d: %s sums %d %d" % (c.name, routes.ROWS[c.row], c.paths, sg.path_variant,
                                                   int(one.astype(np.int64).sum()), int(dD.cpu().numpy().astype(np.int64).sum())), flush=True)
        sg.close()
        pkg.binding.lib().rtdm_debug_sgm_cost16(0)
    sys.exit(0)

# (paths, D, W - D, H)
ROWS = [(8, 64, 61, 23), (8, 128, 61, 23), (5, 96, 44, 18), (4, 96, 44, 18), (8, 272, 20, 12), (5, 1040, 20, 12)]
st = torch.cuda.current_stream().cuda_stream
for paths, D, W1, H in ROWS:
    W = D + W1
    rng = np.random.default_rng(D + paths)
    Ls = rng.integers(0, 256, (3, H, W), dtype=np.uint8)
    Rs = np.roll(Ls, -5, axis=2)
    sg = pkg.HIPSemiGlobalMatcher(numOfDisparities=D, blockSize=5, width=W, height=H, max_batch=3, paths=paths)
    one = sg.compute(Ls[0], Rs[0])
    dD = torch.zeros((3, H, W), dtype=torch.int16, device="cuda")
    sg.compute_device(torch.from_numpy(Ls).cuda(), torch.from_numpy(Rs).cuda(), dD, st)
    torch.cuda.synchronize()
    print("paths %d D %d %dx%d: %s sweeps %d sums %d %d" % (paths, D, W, H, sg.path_variant, sg.pass_stats()[0],
                                                          int(one.astype(np.int64).sum()), int(dD.cpu().numpy().astype(np.int64).sum())), flush=True)
    sg.close()
