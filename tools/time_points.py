"""Times reprojectImageTo3D and the point cloud at 1280x720 (profiles/xyz_time.txt).

  map    rtdm_xyz_map_device on n device frames per call (n = 1, 16, 64): x16 map in, xyz image out
         (2 B read + 12 B written per pixel), missing values handled (the minimum pass runs)
  cloud  rtdm_xyz_cloud_device on the StereoBM's map of a synthetic pair (D 64, 9x9), colour guide, no mask, capacity W * H
         (per pixel 2 B read twice; per kept pixel 3 B read and 16 B written)
  copy   in the same run, a device-to-device copy that moves the same number of bytes (read + written) as the yardstick
and the ratios kernel time / copy time.  Each figure: warm-up, then calls for >= --window seconds, mean per call and per
frame.  --quick: one short pass of every form (for a rocprofv3 --kernel-trace --stats run).

    python tools/time_points.py [--window 1.0] [--quick] [--out FILE]

Writes profiles/xyz_time.txt unless --out names another file (--out "" prints only).
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "xyz_time.txt"))
    a = ap.parse_args()
    import torch
    pkg = importlib.import_module("rt-depth-map_amd")
    W, H, D, w = 1280, 720, 64, 9
    window = 0.05 if a.quick else a.window
    Q = np.array([[1, 0, 0, -W / 2], [0, 1, 0, -H / 2], [0, 0, 0, 700.0], [0, 0, 1 / 2.4, 0.0]])
    L, R = pkg.synth.make_pair(pkg.synth.STREAM_SEED, W, H, D)
    m = pkg.HIPMatcher(numOfDisparities=D, blockSize=w, width=W, height=H)
    disp = m.compute(L, R)
    guide = np.stack([L, R, L], axis=2)
    lines = ["# reprojectImageTo3D and point cloud, %dx%d, StereoBM D %d %dx%d map (%.1f %% invalid), ROUNDED, missing values "
             "handled; %s" % (W, H, D, w, w, 100.0 * float((disp == m.filtered).mean()), torch.cuda.get_device_name(0))]
    sync = torch.cuda.synchronize
    for n in (1, 16, 64):
        rp = pkg.HIPReprojector(Q, W, H, max_batch=n)
        td = torch.tensor(np.broadcast_to(disp, (n, H, W)).copy()).cuda()
        tg = torch.tensor(np.broadcast_to(guide, (n, H, W, 3)).copy()).cuda()
        xyz = torch.empty((n, H, W, 3), dtype=torch.float32, device="cuda")
        pts = torch.empty((n, W * H * 16), dtype=torch.uint8, device="cuda")
        cnt = torch.empty((n,), dtype=torch.int32, device="cuda")
        t_map, k = timed(lambda: rp.map_device(td, d_xyz=xyz), sync, window)
        nbytes = n * W * H * 14
        src, dst = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda"), torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")
        t_copy, _ = timed(lambda: dst.copy_(src), sync, window)
        lines.append("map    n %2d: %8.1f us / call  %7.1f us / frame  (%d calls)   copy moving %d B: %8.1f us   ratio %.2f" % (
            n, t_map * 1e6, t_map * 1e6 / n, k, nbytes, t_copy * 1e6, t_map / t_copy))
        t_cloud, k = timed(lambda: rp.cloud_device(td, pts, cnt, d_guide=tg), sync, window)
        kept = int(cnt.cpu().numpy().sum())
        nbytes = n * W * H * 4 + kept * 19
        src, dst = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda"), torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")
        t_copy, _ = timed(lambda: dst.copy_(src), sync, window)
        lines.append("cloud  n %2d: %8.1f us / call  %7.1f us / frame  (%d calls, %d points / frame)   copy moving %d B: %8.1f us   "
                     "ratio %.2f" % (n, t_cloud * 1e6, t_cloud * 1e6 / n, k, kept // n, nbytes, t_copy * 1e6, t_cloud / t_copy))
        del src, dst, td, tg, xyz, pts, cnt
        rp.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
