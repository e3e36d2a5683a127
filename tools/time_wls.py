"""Times the disparity WLS post-filter at 1280x720 (profiles/wls_time.txt).

  filter      rtdm_wls_filter_device on n device frames per call (n = 1, 16): maps from the left and right StereoBM, gray guide
  end to end  rtdm_bm_compute_filtered: host gray pair in, filtered x16 map out (both matchers, the filter, the copies)
for the headline StereoBM (D 64, 9x9) and the reference's D 192, 13x13.  Each figure: warm-up, then calls for >= --window
seconds, mean per call and per frame.  --quick: one short pass of every form (for a rocprofv3 --kernel-trace --stats run).

    python tools/time_wls.py [--window 1.0] [--quick] [--out FILE]
"""
import argparse
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, sync, window, warmup=3):
    for _ in range(warmup):
        fn()
    sync()
    n, t0 = 0, time.perf_counter()
    while True:
        fn()
        n += 1
        if n % 4 == 0:
            sync()
            if time.perf_counter() - t0 >= window:
                break
    sync()
    return (time.perf_counter() - t0) / n, n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    pkg = importlib.import_module("rt-depth-map_amd")
    W, H = 1280, 720
    window = 0.05 if a.quick else a.window
    lines = ["# WLS post-filter, %dx%d, gray guide, lambda 8000, sigma 1.5, 3 iterations; %s" % (
        W, H, torch.cuda.get_device_name(0))]
    for D, w in ((64, 9), (192, 13)):
        L, R = pkg.synth.make_pair(pkg.synth.STREAM_SEED, W, H, D)
        m = pkg.HIPMatcher(numOfDisparities=D, blockSize=w, width=W, height=H)
        rm = pkg.create_right_matcher(m)
        dL, dR = m.compute(L, R), rm.compute(R, L)
        for n in (1, 16):
            f = pkg.create_disparity_wls_filter(m, max_batch=n)
            tl = torch.tensor(np.broadcast_to(dL, (n, H, W)).copy()).cuda()
            tr = torch.tensor(np.broadcast_to(dR, (n, H, W)).copy()).cuda()
            tg = torch.tensor(np.broadcast_to(L, (n, H, W)).copy()).cuda()
            to = torch.empty((n, H, W), dtype=torch.int16, device="cuda")
            dt, k = timed(lambda: f.filter_device(tl, tr, tg, to), torch.cuda.synchronize, window)
            lines.append("filter      D %3d w %2d  n %2d: %8.1f us / call  %7.1f us / frame  (%d calls)" % (D, w, n, dt * 1e6, dt * 1e6 / n, k))
            f.close()
        f = pkg.create_disparity_wls_filter(m)
        dt, k = timed(lambda: f.compute_filtered(m, rm, L, R), lambda: None, window)
        lines.append("end to end  D %3d w %2d  n  1: %8.1f us / call  (host pair in, filtered map out; %d calls)" % (D, w, dt * 1e6, k))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
