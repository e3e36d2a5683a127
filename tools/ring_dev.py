#!/usr/bin/env python3
"""Development loop for the search kernels on the GPU box: for each configuration check a few frames against the oracle and
time the search stage with HIP events.

    python tools/ring_dev.py [--cfg D,w[,W,H]] ... [--batch 256] [--steps 10]
"""
import argparse, importlib, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cfg", action="append")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=10)
    a = ap.parse_args()
    import numpy as np, torch
    pkg = importlib.import_module("rt-depth-map_amd")
    from oracle import oracle as orc
    orc.build()
    for cfg in a.cfg or ["64,9"]:
        v = [int(x) for x in cfg.split(",")]
        D, w = v[0], v[1]
        W, H = (v[2], v[3]) if len(v) >= 4 else (1280, 720)
        B = a.batch
        dL = torch.empty((B, H, W), dtype=torch.uint8, device="cuda"); dR = torch.empty_like(dL)
        dD = torch.empty((B, H, W), dtype=torch.int16, device="cuda")
        st = torch.cuda.current_stream().cuda_stream
        for i0 in range(0, B, 256):
            n = min(256, B - i0)
            pkg.synth_pairs_device(dL[i0:i0 + n], dR[i0:i0 + n], i0, D, stream=st)
        m = pkg.HIPMatcher(numOfDisparities=D, blockSize=w, width=W, height=H, max_batch=B)
        for _ in range(3): m.compute_device(dL, dR, dD, st)
        torch.cuda.synchronize(); m.set_profiling(True); m.reset_stage_times()
        t0 = time.perf_counter()
        for _ in range(a.steps): m.compute_device(dL, dR, dD, st)
        torch.cuda.synchronize(); dt = time.perf_counter() - t0
        ms = {k: x["total_ms"] / max(1, x["launches"]) for k, x in m.stage_times().items()}
        ok = all(np.array_equal(dD[i].cpu().numpy(), orc.bm_compute(dL[i].cpu().numpy(), dR[i].cpu().numpy(), numDisparities=D, blockSize=w, nthreads=32))
                 for i in sorted({0, B // 2, B - 1}))
        print("cfg %-16s %-16s exact=%-5s %9.1f pairs/s  search %.4f lr %.4f spk %.4f pre %.4f ms" % (
            cfg, m.search_variant, ok, B * a.steps / dt, ms["search"], ms["lrcheck"], ms["speckle"], ms["prefilter"]), flush=True)
        m.close()


if __name__ == "__main__":
    main()
