"""No-GPU checks of the per-object measurements (rtdm_objects_measure_device, rtdm_estimate_batch_measured / _device; rules
G1-G10 of DESIGN.md section 4.18): the symbols and the two struct layouts, every refusal of G10 in its order, the workspace
size, the default params -- and the reference of the GPU tests, tests/measure_ref.py, against per-object Python loops."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import cc_cases as cc
import cc_labels_ref as lr
import measure_ref as mr
import rectify_util as ru
import xyz_ref as xr
from conftest import ROOT, load

NAMES = ("rtdm_measure_default_params rtdm_objects_measure_workspace_bytes rtdm_objects_measure_device "
         "rtdm_estimate_batch_measured rtdm_estimate_batch_measured_device").split()
NULL, BAD_PARAM, BAD_SIZE, NO_DEVICE = -7, -1, -2, -3
Q = ru.calib("320x240")["Q"]


def test_symbols_are_exported_declared_and_bound():
    B = load("binding")
    L = C.CDLL(B.LIB_PATH)
    text = open(os.path.join(ROOT, "include", "rtdm.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for n in NAMES:
        assert hasattr(L, n), "librtdm_hip.so lacks " + n
        assert re.search(r"\b%s\s*\(" % n, text), "include/rtdm.h lacks " + n
        assert n in B.EXPORTS, "binding.EXPORTS lacks " + n
        assert getattr(B.lib(), n).argtypes is not None
    assert B.lib().rtdm_abi_version() == 3
    pkg = load()
    assert C.sizeof(B.ObjectMeasure) == 88 == pkg.MEASURE_DTYPE.itemsize == mr.MEASURE.itemsize
    assert [f[0] for f in B.ObjectMeasure._fields_] == list(pkg.MEASURE_DTYPE.names) == list(mr.MEASURE.names)
    for name in pkg.MEASURE_DTYPE.names:
        assert getattr(B.ObjectMeasure, name).offset == pkg.MEASURE_DTYPE.fields[name][1] == mr.MEASURE.fields[name][1], name
    for f in ("objects_measure_device", "objects_measure_workspace_bytes", "distance_cm", "MeasureParams"):
        assert callable(getattr(pkg, f)), f
    assert pkg.distance_cm([10.0, 4.0], 25.0).tolist() == [25.0, 10.0]
    import inspect
    assert "measure" in inspect.signature(pkg.HIPEstimator.estimate).parameters
    assert {"d_measures", "measure"} <= set(inspect.signature(pkg.HIPEstimator.estimate_device).parameters)
    syms = subprocess.run(["nm", "-DC", os.path.join(ROOT, "rt-depth-map_amd", "lib", "librtdm_host.so")], capture_output=True, text=True).stdout
    assert "rtdm::HIPObjectsCore::estimateBatchMeasured" in syms and "rtdm::HIPObjectsCore::estimateBatch(" in syms


C_CALLER = r"""
#include <stddef.h>
#include <stdio.h>
#include "rtdm.h"
int main(void)
{
    rtdm_measure_params p;
    int (*dev)(int, const rtdm_measure_params*, int, const int16_t*, size_t, size_t, int, int, const double*, const void*, size_t, size_t,
               int, int, const struct rtdm_object*, int, const int*, rtdm_object_measure*, void*, size_t, void*) = rtdm_objects_measure_device;
    rtdm_measure_default_params(&p);
    printf("%d %d %d %d %d %d %d\n", (int)sizeof(rtdm_object_measure), (int)offsetof(rtdm_object_measure, npix),
           (int)offsetof(rtdm_object_measure, nplane), (int)offsetof(rtdm_object_measure, zq), (int)offsetof(rtdm_object_measure, lo),
           (int)offsetof(rtdm_object_measure, hi), (int)offsetof(rtdm_object_measure, mean));
    printf("%d %d %d %d %d\n", (int)sizeof(rtdm_measure_params), (int)offsetof(rtdm_measure_params, disparity_mode),
           (int)offsetof(rtdm_measure_params, max_z), (int)offsetof(rtdm_measure_params, nquant), (int)offsetof(rtdm_measure_params, permille));
    printf("%d %.1f %d %d %d %d\n", p.disparity_mode, p.max_z, p.nquant, p.permille[0], p.permille[1], p.permille[2]);
    return dev && rtdm_objects_measure_workspace_bytes(1, 1, 1, 0) > 0 ? 0 : 1;
}
"""


def test_a_c99_caller_sees_the_layouts_of_ctypes_and_numpy(tmp_path):
    B, pkg = load("binding"), load()
    src = tmp_path / "caller.c"
    src.write_text(C_CALLER)
    libdir = os.path.join(ROOT, "rt-depth-map_amd", "lib")
    exe = str(tmp_path / "caller")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-L", libdir,
                        "-lrtdm_hip", "-Wl,-rpath," + libdir, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    rec, par, dflt = [line.split() for line in run.stdout.strip().splitlines()]
    names = ("npix", "nplane", "zq", "lo", "hi", "mean")
    assert [int(v) for v in rec] == [88] + [getattr(B.ObjectMeasure, n).offset for n in names]
    assert [int(v) for v in rec] == [pkg.MEASURE_DTYPE.itemsize] + [pkg.MEASURE_DTYPE.fields[n][1] for n in names]
    assert [int(v) for v in par] == [C.sizeof(B.MeasureParams)] + [getattr(B.MeasureParams, n).offset
                                                                    for n in ("disparity_mode", "max_z", "nquant", "permille")]
    assert dflt == ["1", "10000.0", "3", "500", "250", "750"]


def test_default_params():
    B, pkg = load("binding"), load()
    p = B.MeasureParams(7, -1.0, 7, (C.c_int * 8)(*[9] * 8))
    B.lib().rtdm_measure_default_params(C.byref(p))
    assert (p.disparity_mode, p.max_z, p.nquant, list(p.permille)) == (B.XYZ_ROUNDED, 1e4, 3, [500, 250, 750, 0, 0, 0, 0, 0])
    B.lib().rtdm_measure_default_params(None)                             # nothing to fill: no crash
    d = pkg.MeasureParams()
    assert (d.disparity_mode, d.max_z, d.permille) == (pkg.XYZ_ROUNDED, 1e4, (500, 250, 750))
    for bad in (dict(disparity_mode=2), dict(max_z=0), dict(max_z=float("inf")), dict(max_z=float("nan")), dict(permille=range(9)),
                dict(permille=[1001]), dict(permille=[-1])):
        with pytest.raises(ValueError):
            pkg.MeasureParams(**bad)
    assert pkg.MeasureParams(permille=()).c.nquant == 0


def test_workspace_size_needs_no_device_and_never_shrinks():
    L = load("binding").lib()
    ws = L.rtdm_objects_measure_workspace_bytes
    assert ws(0, 0, 0, 0) > 0 and ws(-3, -3, -3, 0) > 0
    base = (2, 16, 100, 3)
    for k in range(4):
        sizes = [ws(*[v + (d if j == k else 0) for j, v in enumerate(base)]) for d in range(0, 5)]
        assert sizes == sorted(sizes) and sizes[0] > 0, (k, sizes)
    assert ws(3, 16, 100, 3) > ws(2, 16, 100, 3) and ws(2, 17, 100, 3) > ws(2, 16, 100, 3) and ws(2, 16, 113, 3) > ws(2, 16, 100, 3)


def measure_call(L, B, n=2, disp=True, dpitch=64, dframe=64 * 6, W=20, H=6, Q=True, planes=0, ppitch=96, pplane=96 * 6, labels=1, K=2,
                 objects=True, capacity=4, counts=True, params="default", measures=0, work=True, wbytes=None, **pkw):
    """One rtdm_objects_measure_device call on device 0 whose every argument is in order unless said otherwise (host memory
    everywhere: a call that got as far as a device would be wrong already).  planes / measures: byte offsets, None: absent."""
    buf = np.zeros(1 << 16, np.uint8).ctypes.data
    buf += -buf % 16
    q = (C.c_double * 16)()
    p = None
    if params is not None:
        p = B.MeasureParams()
        L.rtdm_measure_default_params(C.byref(p))
        for k, v in pkw.items():
            if k == "permille":
                p.permille = (C.c_int * 8)(*v)
            else:
                setattr(p, k, v)
    if wbytes is None:
        wbytes = L.rtdm_objects_measure_workspace_bytes(n, capacity, H, 8)
    return L.rtdm_objects_measure_device(0, C.byref(p) if p is not None else None, n, buf if disp else None, dpitch, dframe, W, H,
                                         q if Q else None, buf + planes if planes is not None else None, ppitch, pplane, labels, K,
                                         buf if objects else None, capacity, buf if counts else None,
                                         buf + 32768 + measures if measures is not None else None, buf if work else None, wbytes, None)


def test_every_refusal_comes_before_the_device_and_in_order():
    import torch
    B = load("binding")
    L = B.lib()
    nodev = not torch.cuda.is_available()

    def call(**kw):
        return measure_call(L, B, **kw)

    if nodev:
        assert call() == NO_DEVICE and call(labels=0, ppitch=20, pplane=120) == NO_DEVICE          # nothing wrong but the device
    # D6's list, "mask" read as "plane"
    for missing in ("disp", "Q", "objects", "counts", "work"):
        assert call(**{missing: False}) == NULL, missing
    assert call(planes=None) == NULL
    assert call(n=-1, wbytes=1 << 20) == BAD_SIZE and call(capacity=-1, wbytes=1 << 20) == BAD_SIZE
    for kw in (dict(W=0), dict(H=0), dict(H=-1)):
        assert call(wbytes=1 << 20, **kw) == BAD_SIZE, kw
    assert call(dpitch=65, dframe=65 * 6 + 1) == BAD_SIZE and call(dpitch=38, dframe=38 * 6) == BAD_SIZE
    assert call(labels=0, ppitch=19, pplane=19 * 6) == BAD_SIZE                                  # mask form: below the width
    assert call(ppitch=76, pplane=76 * 6) == BAD_SIZE and call(ppitch=82, pplane=82 * 6) == BAD_SIZE   # L8: label pitch
    assert call(pplane=96 * 6 + 2) == BAD_SIZE
    for off in (1, 2, 3):
        assert call(planes=off) == BAD_SIZE, off
        if nodev:
            assert call(planes=off, labels=0) == NO_DEVICE                                        # mask planes have no alignment
    assert call(dframe=64 * 6 - 2) == BAD_SIZE and call(pplane=96 * 6 - 4) == BAD_SIZE
    assert call(n=1, K=2, pplane=96 * 6 - 4) == BAD_SIZE
    for k in (0, -1, 9):
        assert call(K=k) == BAD_PARAM, k
    # ... then the params and the records: NULL, BAD_PARAM, BAD_SIZE
    assert call(params=None) == NULL and call(measures=None) == NULL
    assert call(K=0, params=None) == BAD_PARAM                            # D6's class count comes before them
    assert call(params=None, disparity_mode=5) == NULL
    for bad in (dict(disparity_mode=2), dict(disparity_mode=-1), dict(max_z=0.0), dict(max_z=-1.0), dict(max_z=float("inf")),
                dict(max_z=float("nan")), dict(nquant=-1), dict(nquant=9), dict(nquant=2, permille=[5, 1001]), dict(nquant=1, permille=[-1])):
        assert call(**bad) == BAD_PARAM, bad
        assert call(measures=4, wbytes=0, **bad) == BAD_PARAM, bad        # ... before the alignment and the workspace
        assert call(measures=None, **bad) == NULL, bad                    # ... and behind the missing records
    for off in (1, 4, 7):
        assert call(measures=off) == BAD_SIZE, off
    need = L.rtdm_objects_measure_workspace_bytes(2, 4, 6, 3)
    assert call(wbytes=need - 1) == BAD_SIZE and call(wbytes=0) == BAD_SIZE
    if nodev:
        assert call(wbytes=need) == NO_DEVICE and call(nquant=2, permille=[5, 1000, 7777]) == NO_DEVICE   # unused entries are not looked at
        assert call(nquant=0) == NO_DEVICE and call(n=1, K=1, pplane=0) == NO_DEVICE
    assert call(n=0) == 0
    assert call(n=0, measures=4) == BAD_SIZE                              # n = 0 is served after the refusals


def test_the_measured_estimator_needs_both_or_neither():
    B = load("binding")
    L = B.lib()
    buf = np.zeros(4096, np.uint8).ctypes.data
    buf += -buf % 16
    q = (C.c_double * 16)()
    rng = (B.HsvRange * 1)(B.HsvRange((C.c_int * 3)(0, 150, 0), (C.c_int * 3)(9, 255, 255)))
    cls = (C.c_int * 1)(0)
    p = B.MeasureParams()
    L.rtdm_measure_default_params(C.byref(p))
    head = [None, 1, buf, 24, 96, buf, 24, 96, q, rng, cls, 1, 1, 1, 1, 25.0, buf, buf, buf, buf, None, 0, 0]
    # no handle: the NULL of the pair comes first, then what rtdm_estimate_batch says of the rest (NULL: the handle)
    assert L.rtdm_estimate_batch_measured(*(head + [C.byref(p), None])) == NULL
    assert L.rtdm_estimate_batch_measured(*(head + [None, buf])) == NULL
    assert L.rtdm_estimate_batch_measured_device(*(head + [None, C.byref(p), None])) == NULL
    assert L.rtdm_estimate_batch_measured_device(*(head + [None, None, buf])) == NULL
    bad = list(head); bad[11] = 0                                         # nranges = 0: BAD_PARAM from the ranges ...
    assert L.rtdm_estimate_batch_measured(*(bad + [C.byref(p), buf])) == BAD_PARAM
    assert L.rtdm_estimate_batch_measured(*(bad + [C.byref(p), None])) == NULL          # ... but behind the pair's NULL
    assert L.rtdm_estimate_batch_measured(*(bad + [None, None])) == L.rtdm_estimate_batch(*bad) == BAD_PARAM


# ---- the reference ------------------------------------------------------------------------------------------------------------
def test_the_key_map_orders_floats():
    v = np.array([-np.inf, -1.0, -0.0, 0.0, 1.0, np.inf], np.float32)
    k = mr.keys(v)
    assert (np.diff(k.astype(np.int64)) > 0).all()
    assert mr.unkeys(k).tobytes() == v.tobytes()
    rng = np.random.default_rng(1)
    r = rng.standard_normal(1000).astype(np.float32) * np.float32(1e3)
    assert np.array_equal(r[np.argsort(mr.keys(r), kind="stable")], np.sort(r)) and mr.unkeys(mr.keys(r)).tobytes() == r.tobytes()


def brute(disp, Q, planes, objects, counts, capacity, labels, mode, max_z, permille):
    """G1-G8 pixel by pixel in Python: sorted() on (sign-aware) floats, one loop per object"""
    H, W = disp.shape
    xyz = xr.reproject(disp, Q, mode, True)
    stored = min(sum(max(int(c), 0) for c in counts), capacity)
    out = []
    for i in range(stored):
        x, y, w, h, cls = objects[i]
        rec = dict(npix=0, nplane=0, zq=[0.0] * 8, lo=[0.0] * 3, hi=[0.0] * 3, mean=[0.0] * 3)
        out.append(rec)
        if not 0 <= cls < len(planes) or w <= 0 or h <= 0:
            continue
        pts = []
        for yy in range(max(y, 0), min(y + h, H)):
            for xx in range(max(x, 0), min(x + w, W)):
                v = int(planes[cls][yy, xx])
                if (v == i + 1) if labels else (v != 0):
                    rec["nplane"] += 1
                    z = float(xyz[yy, xx, 2])
                    if abs(z - 10000.0) >= xr.FLT_EPSILON and abs(z) <= max_z:
                        pts.append(tuple(float(c) for c in xyz[yy, xx]))
        rec["npix"] = len(pts)
        if not pts:
            continue
        order = lambda v: (v, math.copysign(1.0, v))                         # -0.0 below +0.0
        zs = sorted((p[2] for p in pts), key=order)
        rec["zq"] = [zs[((len(pts) - 1) * p) // 1000] for p in permille] + [0.0] * (8 - len(permille))
        for j in range(3):
            col = [p[j] for p in pts]
            rec["lo"][j], rec["hi"][j] = min(col, key=order), max(col, key=order)
            rec["mean"][j] = math.fsum(col) / len(pts)
    return out


@pytest.mark.parametrize("mode", [xr.ROUNDED, xr.FIXED16])
@pytest.mark.parametrize("labels", [True, False])
def test_reference_against_brute_force(mode, labels):
    rng = np.random.default_rng(11 + mode)
    W, H, K, cap = 23, 9, 2, 8
    disp = (rng.integers(-40, 900, (H, W))).astype(np.int16)
    disp[rng.random((H, W)) < 0.15] = -16
    planes = rng.choice(np.array([0, 1, 2, 4, 8, 255], np.int32), (K, H, W))
    if not labels:
        planes = planes.astype(np.uint8)
    objects = [(0, 0, W, H, 0), (-3, -2, 9, 6, 1), (5, 2, 1, 1, 0), (20, 7, 30, 30, 1), (4, 4, 0, 3, 0), (2, 2, 5, 5, 7), (30, 1, 4, 4, 0),
               (6, 0, 7, 9, 1)]
    counts = [5, 3]
    q = np.array(Q, np.float64).copy()
    q[3, 3] = -3.0 * q[3, 2]                                                  # both signs of Z
    for max_z in (1e4, 150.0):
        got = mr.measure_frame(disp, q, planes, objects, counts, cap, labels, mode, max_z)
        want = brute(disp, q, planes, objects, counts, cap, labels, mode, max_z, mr.ALL_PERMILLE)
        assert len(got) == len(want) == 8
        for i, w in enumerate(want):
            assert int(got[i]["npix"]) == w["npix"] and int(got[i]["nplane"]) == w["nplane"], i
            for name in ("zq", "lo", "hi"):
                assert got[i][name].tobytes() == np.array(w[name], np.float32).tobytes(), (i, name)
            assert got[i]["mean"].tobytes() == np.array(w["mean"], np.float64).tobytes(), i
        assert sum(w["npix"] > 0 for w in want) >= 3 and [w["npix"] for w in want][4:7] == [0, 0, 0]
        assert any(w["lo"][2] < 0 < w["hi"][2] for w in want)


def test_the_hostile_masks_give_meaningful_objects():
    """What tests/test_gpu_measure.py relies on: the objects of its three masks are mostly non-empty under the ramp map."""
    import test_gpu_objects_labels as tl
    for name, total, least in (("rings_cut_outer2-257x131", 17, 17), ("noise45-257x131", 145, 130), ("dots-257x131", 8320, 7000)):
        m = cc.BY_NAME[name]
        H, W = m.shape
        fr = lr.frame([m], 1, True, 9000)
        assert fr["stored"] == total
        rec = mr.measure_frame(tl.ramp_map(W, H, 5), Q, fr["labels"], fr["objects"], fr["counts"], 9000, True, permille=(0, 500, 1000))
        assert int((rec["npix"] > 0).sum()) >= least, name
        assert np.array_equal(rec["nplane"], fr["stats"][:, 0])               # unclipped boxes: the label count is m00
        if name.startswith("noise"):
            assert int(rec["npix"].max()) == 12439
        if name.startswith("dots"):
            one = rec[rec["npix"] == 1]
            assert len(one) >= least and (one["zq"][:, 0] == one["zq"][:, 2]).all() and (one["lo"][:, 2] == one["zq"][:, 1]).all()
