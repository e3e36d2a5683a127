"""Times the rectifier's set-up at 1280x720 on the 1280x720 calibration (profiles/rectify_calib_time.txt): the two calibration
files -> a ready rtdm_rectify handle,

  calib   rtdm_calib_load + rtdm_stereo_rectify (alpha -1, ZERO_DISPARITY) + rtdm_rectify_create_calib: the maps are built on
          the device (k_rectmap_walk, k_rectmap_pixel) and never exist on the host
  maps    the route the parent commit offers: the same load and stereoRectify, both cameras' maps by the CPU oracle
          (orc_init_undistort_rectify_map) on the host, then rtdm_rectify_create, which crops and uploads them

with the crop the reference derives from the files (main.cpp:80-85).  The two routes alternate in one process; each figure is
the median (and the minimum) of --reps set-ups after --warmup untimed ones, on a host clock: both create calls return only
when the handle is ready.  The shares of the steps of each route are medians too.  Both handles are checked to rectify one
frame pair to the same bytes.  --kernel-stats CSV adds the two kernels alone from a kernel_stats.csv that
`rocprofv3 --kernel-trace --stats --output-format csv -- python tools/time_rectify_setup.py --quick --out ""` wrote in a run
of its own.

    python tools/time_rectify_setup.py [--reps 25] [--warmup 3] [--quick] [--kernel-stats CSV] [--out FILE]

Writes profiles/rectify_calib_time.txt unless --out names another file (--out "" prints only).
"""
import argparse
import csv
import ctypes as C
import importlib
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
RES = "1280x720"
YML = os.path.join(ROOT, "tests", "golden", "calib_yml", RES)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--kernel-stats", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rectify_calib_time.txt"))
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "this tool measures on the GPU; there is nothing to time without one"
    pkg = importlib.import_module("rt-depth-map_amd")
    from oracle import oracle as orc
    orc.build()
    B = pkg.binding
    L = B.lib()
    intr, extr = os.path.join(YML, "intrinsics.yml").encode(), os.path.join(YML, "extrinsics.yml").encode()
    reps, warmup = (3, 1) if a.quick else (a.reps, a.warmup)
    clock = time.perf_counter

    def load_and_rectify():
        c, stored, mask, r = B.Calib(), B.Rectification(), C.c_uint(0), B.Rectification()
        B.check(L.rtdm_calib_load(intr, extr, C.byref(c), C.byref(stored), C.byref(mask)), "rtdm_calib_load")
        B.check(L.rtdm_stereo_rectify(C.byref(c), B.CALIB_ZERO_DISPARITY, -1.0, 0, 0, C.byref(r)), "rtdm_stereo_rectify")
        r1, r2 = stored.roi1, stored.roi2
        roi = (max(r1.x, r2.x), max(r1.y, r2.y), min(r1.width, r2.width), min(r1.height, r2.height))
        return c, r, roi

    def route_calib():
        t0 = clock()
        c, r, roi = load_and_rectify()
        t1 = clock()
        h = C.c_void_p()
        B.check(L.rtdm_rectify_create_calib(C.byref(c), C.byref(r), *roi, 1, 0, C.byref(h)), "rtdm_rectify_create_calib")
        t2 = clock()
        return h, roi, (t2 - t0, t1 - t0, 0.0, t2 - t1)

    def route_maps():
        t0 = clock()
        c, r, roi = load_and_rectify()
        t1 = clock()
        W, H = c.width, c.height
        maps = []
        for M, D, R, P in ((c.M1, c.D1, r.R1, r.P1), (c.M2, c.D2, r.R2, r.P2)):
            maps += orc.init_undistort_rectify_map(np.array(M).reshape(3, 3), np.array(D), np.array(R).reshape(3, 3),
                                                   np.array(P).reshape(3, 4), W, H)
        t2 = clock()
        h = C.c_void_p()
        B.check(L.rtdm_rectify_create(maps[0].ctypes.data, maps[1].ctypes.data, maps[2].ctypes.data, maps[3].ctypes.data, W, H,
                                      *roi, 1, 0, C.byref(h)), "rtdm_rectify_create")
        t3 = clock()
        return h, roi, (t3 - t0, t1 - t0, t2 - t1, t3 - t2)

    def rectified(h, roi, left, right):
        l, r = np.empty((roi[3], roi[2]), np.uint8), np.empty((roi[3], roi[2]), np.uint8)
        B.check(L.rtdm_rectify_gray(h, left.ctypes.data, left.strides[0], right.ctypes.data, right.strides[0], l.ctypes.data,
                                    roi[2], r.ctypes.data, roi[2]), "rtdm_rectify_gray")
        return l, r

    times = {"calib": [], "maps": []}
    same = None
    for i in range(warmup + reps):
        for name, route in (("calib", route_calib), ("maps", route_maps)) if i % 2 == 0 else (("maps", route_maps), ("calib", route_calib)):
            h, roi, t = route()
            if i >= warmup:
                times[name].append(t)
            if i == 0:
                W, H = 1280, 720
                la, ra = pkg.synth.make_pair(pkg.synth.STREAM_SEED + 11, W, H, 16)
                left, right = np.ascontiguousarray(np.stack([la, ra, la], -1)), np.ascontiguousarray(np.stack([ra, la, ra], -1))
                out = rectified(h, roi, left, right)
                same = out if same is None else (np.array_equal(same[0], out[0]) and np.array_equal(same[1], out[1]))
            L.rtdm_rectify_destroy(h)
    assert same is True, "the two routes rectify a frame pair differently"

    def med(name, k):
        return statistics.median(t[k] for t in times[name]) * 1e3

    lines = ["# files -> ready rtdm_rectify handle, %s calibration, crop %dx%d at (%d, %d), max_batch 1; %d set-ups per route, "
             "alternating, after %d warm-up; %s" % (RES, roi[2], roi[3], roi[0], roi[1], reps, warmup, torch.cuda.get_device_name(0))]
    for name, what in (("calib", "maps built on the device (rtdm_rectify_create_calib)"),
                       ("maps", "oracle maps on the host + rtdm_rectify_create")):
        lines.append("%-5s  median %8.3f ms  min %8.3f ms   load + stereoRectify %6.3f   host maps %8.3f   create %7.3f   %s" % (
            name, med(name, 0), min(t[0] for t in times[name]) * 1e3, med(name, 1), med(name, 2), med(name, 3), what))
    ratio = med("maps", 0) / med("calib", 0)
    lines.append("the new route is %s: %.2fx (median over median); both handles rectify a frame pair to the same bytes" % (
        "the faster of the two" if ratio > 1 else "NOT the faster of the two", ratio))
    if a.kernel_stats:
        rows = [r for r in csv.DictReader(open(a.kernel_stats)) if "k_rectmap" in r["Name"]]
        lines.append("# the two kernels alone (rocprofv3 --kernel-trace --stats, a run of its own; roi form, one launch per camera)")
        for r in rows:
            lines.append("%-16s calls %4s   average %8.1f us   min %8.1f us   max %8.1f us" % (
                r["Name"].split("(")[0].replace("rtdm::", "").replace("void ", ""), r["Calls"], float(r["AverageNs"]) / 1e3,
                float(r["MinNs"]) / 1e3, float(r["MaxNs"]) / 1e3))
        if not rows:
            lines.append("not measured: %s holds no k_rectmap line" % os.path.basename(a.kernel_stats))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
