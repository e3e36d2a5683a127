"""No-GPU checks of the detector's label planes, pixel moments and own-pixel depth (rtdm_objects_detect_labels_device / _batch,
rtdm_depth_objects_labels_device, rtdm_estimator_set_own_pixels / _get_own_pixels; rules L1-L8 of DESIGN.md section 4.17).

The reference of the GPU tests, tests/cc_labels_ref.py, is anchored here: on every mask of tests/cc_cases.py its kept boxes are
the CPU oracle's, its labelled pixels lie in the foreground and its moments count them.  The masks and the scene that keep the
depth tests from going soft are pinned too: they DO hold objects whose boxes contain foreign foreground of their class.

Not here: the refusals that are measured against a live detector (label pitch against the width, plane strides against the
height): no handle exists without a device, so tests/test_gpu_objects_labels.py::test_refusals_that_need_the_handle has them."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import cc_cases as cc
import cc_labels_ref as lr
import labels_scene as ls
import rectify_util as ru
from conftest import ROOT, load

NAMES = ("rtdm_objects_detect_labels_device rtdm_objects_detect_labels_batch rtdm_depth_objects_labels_device "
         "rtdm_estimator_set_own_pixels rtdm_estimator_get_own_pixels").split()
NULL, BAD_PARAM, BAD_SIZE, NO_DEVICE = -7, -1, -2, -3
SETTINGS = [(zb, area) for zb in (True, False) for area in (1, 12)]


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
    assert "typedef struct rtdm_object_stats { int64_t m00, m10, m01, m20, m11, m02; } rtdm_object_stats;" in text
    pkg = load()
    assert C.sizeof(B.ObjectStats) == 48 and pkg.STATS_DTYPE.itemsize == 48
    assert [f[0] for f in B.ObjectStats._fields_] == list(pkg.STATS_DTYPE.names) == list(lr.MOMENTS)
    # L3: what stays as it is
    assert B.lib().rtdm_abi_version() == 3 and "#define RTDM_MAX_REGIONS 64" in text
    assert "typedef struct rtdm_object { int x, y, width, height, cls, first_pixel, reserved[2]; } rtdm_object;" in text
    assert C.sizeof(B.Object) == 32
    assert all(callable(getattr(pkg.HIPObjectDetector, m)) for m in ("detect_labels", "detect_labels_device"))
    assert callable(pkg.depth_objects_labels_device) and callable(pkg.centroids)
    assert isinstance(pkg.HIPEstimator.own_pixels, property)


C_CALLER = r"""
#include "rtdm.h"
int main(void)
{
    int (*dev)(rtdm_objects*, int, const uint8_t*, size_t, size_t, const rtdm_hsv_range*, const int*, int, int, int, int, uint8_t*, size_t,
               size_t, rtdm_object*, int, int*, rtdm_region*, int32_t*, size_t, size_t, rtdm_object_stats*, void*) =
        rtdm_objects_detect_labels_device;
    int (*batch)(rtdm_objects*, int, const uint8_t*, size_t, size_t, const rtdm_hsv_range*, const int*, int, int, int, int, uint8_t*, size_t,
                 size_t, rtdm_object*, int, int*, rtdm_region*, int32_t*, size_t, size_t, rtdm_object_stats*) =
        rtdm_objects_detect_labels_batch;
    int (*depth)(int, int, const int16_t*, size_t, size_t, int, int, const double*, const int32_t*, size_t, size_t, int,
                 const rtdm_object*, int, const int*, double, double*, int*, void*, size_t, void*) = rtdm_depth_objects_labels_device;
    int (*set)(rtdm_estimator*, int) = rtdm_estimator_set_own_pixels;
    int (*get)(const rtdm_estimator*, int*) = rtdm_estimator_get_own_pixels;
    int on = 7;
    return (sizeof(rtdm_object_stats) == 48 && dev && batch && depth && set(0, 1) == RTDM_ERR_NULL && get(0, &on) == RTDM_ERR_NULL &&
            on == 7) ? 0 : 1;
}
"""


def test_a_c99_caller_sees_48_bytes_of_moments(tmp_path):
    src = tmp_path / "caller.c"
    src.write_text(C_CALLER)
    libdir = os.path.join(ROOT, "rt-depth-map_amd", "lib")
    exe = str(tmp_path / "caller")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-L", libdir,
                        "-lrtdm_hip", "-Wl,-rpath," + libdir, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr


# ---- the reference ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cc.NAMES)
def test_reference_against_the_oracle(oracle, name):
    m = cc.BY_NAME[name]
    for zb, area in SETTINGS:
        fr = lr.frame([m], area, zb)
        assert [o[:4] for o in fr["objects"]] == oracle.external_boxes(m, area, zb, max_boxes=1 << 16), (zb, area)
        lab = fr["labels"][0]
        fg = m != 0
        if zb:
            fg = fg.copy(); fg[0, :] = fg[-1, :] = False; fg[:, 0] = fg[:, -1] = False
        assert not (lab[~fg] != 0).any()                                     # labelled pixels are foreground
        assert int(fr["stats"][:, 0].sum()) == int((lab != 0).sum())            # and the moments count exactly them
        assert set(np.unique(lab).tolist()) == set(range(0 if (lab == 0).any() else 1, fr["stored"] + 1))
        for i, (x, y, w, h, _) in enumerate(fr["objects"]):
            if i % 97 == 0:                                                  # a sample: the box of the labelled pixels is the object's
                ys, xs = np.nonzero(lab == i + 1)
                assert (xs.min(), ys.min(), xs.max() - xs.min() + 1, ys.max() - ys.min() + 1) == (x, y, w, h)
                assert ys.min() * m.shape[1] + xs[ys == ys.min()].min() == fr["first_pixels"][i]


def test_moments_by_hand():
    m = np.zeros((6, 9), np.uint8)
    m[1, 2:5] = 255; m[2, 4] = 255                       # one component: (2,1) (3,1) (4,1) (4,2)
    m[4, 7] = 255                                        # another
    fr = lr.frame([m], 1, False)
    assert fr["objects"] == [(7, 4, 1, 1, 0), (2, 1, 3, 2, 0)]
    assert fr["stats"].tolist() == [[1, 7, 4, 49, 28, 16], [4, 13, 5, 45, 17, 7]]
    assert lr.frame([m], 1, False, capacity=1)["labels"].sum() == 1          # the second object did not fit: its pixels read 0
    pkg = load()
    st = np.zeros(2, pkg.STATS_DTYPE)
    for k, name in enumerate(lr.MOMENTS):
        st[name] = fr["stats"][:, k]
    assert pkg.centroids(st).tolist() == [[7.0, 4.0], [13 / 4, 5 / 4]]
    assert np.isnan(pkg.centroids(np.zeros(1, pkg.STATS_DTYPE))).all()
    with pytest.raises(ValueError):
        pkg.centroids(np.zeros((2, 6), np.int64))


@pytest.mark.parametrize("name,kept", [("rings_cut_outer2-257x131", 17)])
def test_every_box_of_the_cut_rings_holds_foreign_foreground(name, kept):
    m = cc.BY_NAME[name]
    for zb, area in SETTINGS:
        fr = lr.frame([m], area, zb)
        assert fr["stored"] == kept
        assert lr.contaminated([m], fr["labels"], fr["objects"], fr["stored"]) == [True] * kept, (zb, area)


def test_the_quilt_has_a_thousand_contaminated_boxes():
    m = cc.BY_NAME["quilt5-384x384"]
    fr = lr.frame([m], 1, True)
    bad = lr.contaminated([m], fr["labels"], fr["objects"], fr["stored"])
    assert fr["stored"] == 5329 and sum(bad) >= 1000 and not all(bad)
    m = cc.BY_NAME["noise45-257x131"]
    fr = lr.frame([m], 1, True)
    bad = lr.contaminated([m], fr["labels"], fr["objects"], fr["stored"])
    assert fr["stored"] == 145 and 0 < sum(bad) < 145                       # both kinds: contaminated and clean boxes


def test_the_estimator_scene_keeps_two_objects_of_one_class(oracle):
    c, maps = ru.maps(oracle, "320x240")
    left, _ = ls.pair(c)
    want = ls.detect(oracle, c, maps, left)                                  # after oracle.morph_open_close
    assert want["counts"] == [2]
    fr = lr.frame(want["masks"], ls.MIN_AREA, True, 16)
    assert [o[:4] for o in fr["objects"]] == [o[:4] for o in want["objects"]]
    (sx, sy, sw, sh, _), (lx, ly, lw, lh, _) = fr["objects"]                 # the square comes first: its first pixel is the later one
    assert lx <= sx and ly <= sy and sx + sw <= lx + lw and sy + sh <= ly + lh, "the square's pixels lie inside the L's box"
    assert lr.contaminated(want["masks"], fr["labels"], fr["objects"], 2) == [False, True]
    assert fr["stats"][0, 0] > 500 and fr["stats"][1, 0] > 2000


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def ranges_of(B, n):
    return (B.HsvRange * max(n, 1))(*[B.HsvRange((C.c_int * 3)(0, 150, 0), (C.c_int * 3)(9, 255, 255)) for _ in range(n)])


def ints(*v):
    return (C.c_int * max(len(v), 1))(*v)


@pytest.mark.parametrize("device", [True, False])
def test_the_labels_detector_refuses_as_the_detector_does(device):
    """L8: the refusals of rtdm_objects_detect_device in its order -- as far as no handle is needed; whatever is said of the
    label planes and the moments comes behind the handle."""
    B = load("binding")
    L = B.lib()
    buf = np.zeros(8192, np.uint8).ctypes.data

    def call(n=1, rgb=True, nranges=2, classes=(0, 1), nclasses=2, ranges=True, cls=True, objects=True, capacity=4, counts=True, rois=True,
             labels=buf, lpitch=32, lplane=128, stats=buf + 4096):
        args = [None, n, buf if rgb else None, 24, 96, ranges_of(B, nranges) if ranges else None, ints(*classes) if cls else None, nranges,
                nclasses, 1, 1, None, 0, 0, buf if objects else None, capacity, buf if counts else None, buf if rois else None,
                labels, lpitch, lplane, stats]
        return L.rtdm_objects_detect_labels_device(*(args + [None])) if device else L.rtdm_objects_detect_labels_batch(*args)

    assert call() == NULL                                    # nothing wrong but the handle
    for missing in ("rgb", "ranges", "cls", "counts", "rois", "objects"):
        assert call(**{missing: False}) == NULL, missing
    for nr in (0, -1, 17):
        assert call(nranges=nr, classes=(0,) * 17, nclasses=1) == BAD_PARAM, nr
    for k in (0, -1, 9):
        assert call(nclasses=k) == BAD_PARAM, k
    assert call(classes=(0, 2)) == BAD_PARAM and call(classes=(1, 1)) == BAD_PARAM
    assert call(n=-1) == BAD_SIZE and call(capacity=-1) == BAD_SIZE
    # the handle is asked for before the label planes: a misaligned plane, an odd pitch, no outputs at all -- NULL every time
    assert call(labels=buf + 1) == NULL and call(lpitch=33) == NULL and call(stats=buf + 4) == NULL
    assert call(labels=None, stats=None) == NULL and call(n=0) == NULL


def depth_call(L, n=2, disp=True, dpitch=64, dframe=64 * 6, W=20, H=6, Q=True, labels=0, lpitch=96, lplane=96 * 6, K=2, objects=True,
               capacity=4, counts=True, mean=True, npix=True, work=True, wbytes=None):
    """One rtdm_depth_objects_labels_device call on device 0 whose every argument is in order unless said otherwise (host
    memory everywhere: a call that got as far as a device would be wrong already).  labels: byte offset of the planes, None: absent."""
    buf = np.zeros(1 << 16, np.uint8).ctypes.data
    buf += -buf % 16
    q = (C.c_double * 16)()
    if wbytes is None:
        wbytes = L.rtdm_depth_objects_workspace_bytes(n, capacity, H)
    return L.rtdm_depth_objects_labels_device(0, n, buf if disp else None, dpitch, dframe, W, H, q if Q else None,
                                              buf + labels if labels is not None else None, lpitch, lplane, K, buf if objects else None,
                                              capacity, buf if counts else None, 25.0, buf if mean else None, buf if npix else None,
                                              buf if work else None, wbytes, None)


def test_every_refusal_of_the_labels_depth_call_comes_before_the_device():
    import torch
    L = load("binding").lib()
    nodev = not torch.cuda.is_available()
    if nodev:
        assert depth_call(L) == NO_DEVICE                                # nothing wrong but the missing device
    for missing in ("disp", "Q", "objects", "counts", "mean", "npix", "work"):
        assert depth_call(L, **{missing: False}) == NULL, missing
    assert depth_call(L, labels=None) == NULL
    assert depth_call(L, n=-1, wbytes=1 << 20) == BAD_SIZE and depth_call(L, capacity=-1, wbytes=1 << 20) == BAD_SIZE
    for kw in (dict(W=0), dict(H=0), dict(H=-1)):
        assert depth_call(L, wbytes=1 << 20, **kw) == BAD_SIZE, kw
    assert depth_call(L, dpitch=65, dframe=65 * 6 + 1) == BAD_SIZE       # D6 as before: odd pitch
    assert depth_call(L, dpitch=38, dframe=38 * 6) == BAD_SIZE           # below 2 * width
    assert depth_call(L, lpitch=76, lplane=76 * 6) == BAD_SIZE           # "mask" read as "label": below 4 * width
    assert depth_call(L, lpitch=79, lplane=79 * 6) == BAD_SIZE
    assert depth_call(L, lpitch=82, lplane=82 * 6) == BAD_SIZE           # wide enough, but no multiple of 4
    assert depth_call(L, lplane=96 * 6 + 2) == BAD_SIZE                  # a plane stride that is no multiple of 4
    for off in (1, 2, 3):
        assert depth_call(L, labels=off) == BAD_SIZE, off                # planes that are not 4-byte aligned
    assert depth_call(L, dframe=64 * 6 - 2) == BAD_SIZE                  # frame 1 would begin inside frame 0
    assert depth_call(L, lplane=96 * 6 - 4) == BAD_SIZE                  # ... and plane 1 inside plane 0
    assert depth_call(L, n=1, K=2, lplane=96 * 6 - 4) == BAD_SIZE        # one frame, yet two planes
    for k in (0, -1, 9):
        assert depth_call(L, K=k) == BAD_PARAM, k
    need = L.rtdm_depth_objects_workspace_bytes(2, 4, 6)                 # D5: one workspace size serves both calls
    assert depth_call(L, wbytes=need - 1) == BAD_SIZE and depth_call(L, wbytes=0) == BAD_SIZE
    if nodev:
        assert depth_call(L, lpitch=80, lplane=80 * 6) == NO_DEVICE and depth_call(L, labels=4) == NO_DEVICE
        assert depth_call(L, n=1, K=1, lplane=0) == NO_DEVICE
    assert depth_call(L, n=0) == 0


def test_the_own_pixels_switch_needs_an_estimator():
    L = load("binding").lib()
    on = C.c_int(7)
    assert L.rtdm_estimator_set_own_pixels(None, 1) == NULL and L.rtdm_estimator_set_own_pixels(None, 0) == NULL
    assert L.rtdm_estimator_get_own_pixels(None, C.byref(on)) == NULL and on.value == 7


def test_host_library_exports_the_pass_throughs():
    lib = os.path.join(ROOT, "rt-depth-map_amd", "lib", "librtdm_host.so")
    syms = subprocess.run(["nm", "-DC", lib], capture_output=True, text=True).stdout
    for name in ("detectLabelsDevice", "setOwnPixels"):
        assert "rtdm::HIPObjectsCore::" + name in syms, name
