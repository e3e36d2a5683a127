"""No-GPU checks of the batched, multi-class object detection (rtdm_objects_create_batch, rtdm_objects_detect_device,
rtdm_objects_detect_batch, rtdm_estimate_frame_classes; rules O1-O6 of DESIGN.md section 4.15): the symbols are exported,
declared and bound, every refusal that needs no device is made before one is looked for, and tests/objects_batch_ref.py with
one class and one range is the oracle's single-mask chain.

Not here: the refusals that are measured against a live handle -- a pitch below 3 * width, a mask pitch below width, frame or
plane strides that make planes overlap, more classes than the handle's max_classes.  No handle exists without a device, so
tests/test_gpu_objects_batch.py::test_refusals_that_need_the_handle checks them."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import cc_cases as cc
import objects_batch_ref as ref
from conftest import ROOT, load

NAMES = "rtdm_objects_create_batch rtdm_objects_detect_device rtdm_objects_detect_batch rtdm_estimate_frame_classes".split()
NULL, BAD_PARAM, BAD_SIZE, UNSUPPORTED, NO_DEVICE = -7, -1, -2, -6, -3


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
    for word in ("#define RTDM_MAX_HSV_RANGES 16", "#define RTDM_MAX_CLASSES 8",
                 "typedef struct rtdm_object { int x, y, width, height, cls, first_pixel, reserved[2]; } rtdm_object;"):
        assert word in text, word
    pkg = load()
    assert C.sizeof(B.Object) == 32 and pkg.OBJECT_DTYPE.itemsize == 32
    assert [f[0] for f in B.Object._fields_] == list(pkg.OBJECT_DTYPE.names)
    assert (B.MAX_HSV_RANGES, B.MAX_CLASSES, B.MAX_REGIONS) == (16, 8, 64) and "#define RTDM_MAX_REGIONS 64" in text
    assert B.lib().rtdm_abi_version() == 3
    assert callable(pkg.estimate_frame_classes) and callable(pkg.HIPObjectDetector.detect_classes) and callable(pkg.HIPObjectDetector.detect_device)


def test_create_validates_before_it_looks_for_a_device():
    L = load("binding").lib()
    h = C.c_void_p()
    assert L.rtdm_objects_create_batch(64, 48, 1, 1, 0, None) == NULL
    for w, hh in ((0, 48), (64, 0), (-1, 48), (40000, 4)):
        assert L.rtdm_objects_create_batch(w, hh, 1, 1, 0, C.byref(h)) == BAD_SIZE, (w, hh)
    for mb in (0, -1, 65):
        assert L.rtdm_objects_create_batch(64, 48, mb, 1, 0, C.byref(h)) == BAD_SIZE, mb
    for mc in (0, -1, 9):
        assert L.rtdm_objects_create_batch(64, 48, 1, mc, 0, C.byref(h)) == BAD_PARAM, mc
    assert L.rtdm_objects_create_batch(8193, 4, 1, 1, 0, C.byref(h)) == UNSUPPORTED
    import torch
    if not torch.cuda.is_available():
        assert L.rtdm_objects_create_batch(64, 48, 64, 8, 0, C.byref(h)) == NO_DEVICE      # the limits themselves are served
        assert L.rtdm_objects_create_batch(8192, 4, 1, 1, 0, C.byref(h)) == NO_DEVICE
        assert L.rtdm_objects_create(64, 48, 0, C.byref(h)) == NO_DEVICE


def ranges_of(B, n):
    return (B.HsvRange * max(n, 1))(*[B.HsvRange((C.c_int * 3)(0, 150, 0), (C.c_int * 3)(9, 255, 255)) for _ in range(n)])


def ints(*v):
    return (C.c_int * max(len(v), 1))(*v)


def batch_call(L, B, device, ob=None, n=1, rgb=True, nranges=2, classes=(0, 1), nclasses=2, ranges=True, cls=True, objects=True,
               capacity=4, counts=True, rois=True):
    """One call of rtdm_objects_detect_device / _batch on 8 x 4 frames whose every argument is in order unless said otherwise."""
    buf = np.zeros(4096, np.uint8).ctypes.data
    args = [ob, n, buf if rgb else None, 24, 96, ranges_of(B, nranges) if ranges else None, ints(*classes) if cls else None, nranges,
            nclasses, 1, 1, None, 0, 0, buf if objects else None, capacity, buf if counts else None, buf if rois else None]
    return L.rtdm_objects_detect_device(*(args + [None])) if device else L.rtdm_objects_detect_batch(*args)


@pytest.mark.parametrize("device", [True, False])
def test_refusals_of_the_batched_calls_without_a_handle(device):
    B = load("binding")
    L = B.lib()
    call = lambda **kw: batch_call(L, B, device, **kw)       # noqa: E731
    assert call() == NULL                                    # nothing wrong but the handle
    for missing in ("rgb", "ranges", "cls", "counts", "rois", "objects"):
        assert call(**{missing: False}) == NULL, missing
    assert call(objects=False, capacity=0) == NULL           # ... which is only needed with a capacity (the handle again)
    for nr in (0, -1, 17):
        assert call(nranges=nr, classes=(0,) * 17, nclasses=1) == BAD_PARAM, nr
    for k in (0, -1, 9):
        assert call(nclasses=k) == BAD_PARAM, k
    assert call(classes=(0, -1)) == BAD_PARAM                # a class id outside [0, nclasses)
    assert call(classes=(0, 2)) == BAD_PARAM
    assert call(classes=(0, 0)) == BAD_PARAM                 # class 1 owns no range
    assert call(classes=(1, 1)) == BAD_PARAM
    assert call(nranges=3, classes=(0, 2, 2), nclasses=3) == BAD_PARAM
    assert call(nranges=16, classes=tuple(range(8)) * 2, nclasses=8) == NULL          # the limits themselves pass
    assert call(n=-1) == BAD_SIZE
    assert call(capacity=-1) == BAD_SIZE
    assert call(n=0) == NULL                                 # n = 0 is no excuse for a missing handle


def test_refusals_of_the_chain_without_handles():
    B = load("binding")
    L = B.lib()
    buf = np.zeros(4096, np.uint8).ctypes.data
    q = (C.c_double * 16)()
    mean, cnt, n = (C.c_double * 4)(), (C.c_int * 4)(), C.c_int()

    def call(rgb=buf, Q=q, ranges=ranges_of(B, 2), cls=ints(0, 1), nranges=2, nclasses=2, objects=buf, nobj=C.byref(n)):
        return L.rtdm_estimate_frame_classes(None, None, None, rgb, 24, buf, 24, Q, ranges, cls, nranges, nclasses, 1, 1, 25.0, objects,
                                             mean, cnt, 4, nobj, None, 0)

    assert call() == NULL
    for kw in (dict(rgb=None), dict(Q=None), dict(ranges=None), dict(cls=None), dict(objects=None), dict(nobj=None)):
        assert call(**kw) == NULL, kw
    assert call(nranges=0) == BAD_PARAM and call(nranges=17) == BAD_PARAM
    assert call(nclasses=0) == BAD_PARAM and call(nclasses=9) == BAD_PARAM
    assert call(cls=ints(0, 2)) == BAD_PARAM and call(cls=ints(1, 1)) == BAD_PARAM


def test_python_layer_raises_for_wrong_arguments():
    pkg = load()
    with pytest.raises(pkg.binding.RtdmError) as e:
        pkg.HIPObjectDetector(64, 48, max_batch=65)
    assert e.value.status == BAD_SIZE
    with pytest.raises(pkg.binding.RtdmError) as e:
        pkg.HIPObjectDetector(64, 48, max_classes=9)
    assert e.value.status == BAD_PARAM
    from importlib import import_module
    m = import_module(pkg.__name__ + ".objects")
    with pytest.raises(ValueError):
        m._hsv_classes([ref.R_RED, ref.R_BLUE], [0])
    rng, cls, nr, K = m._hsv_classes([ref.R_RED, ref.R_BLUE, ref.R_GREEN], None)
    assert (nr, K, list(cls)) == (3, 3, [0, 1, 2]) and list(rng[1].low) == [110, 150, 0] and list(rng[2].high) == [70, 255, 255]
    assert m._hsv_classes(ref.TWO_RANGES, ref.TWO_CLASSES)[2:] == (4, 2)


def test_reference_with_one_class_and_one_range_is_the_single_mask_chain(oracle):
    rgb = cc.hsv_frame()
    for lo, hi in (oracle.HSV_LOW, oracle.HSV_HIGH), ((20, 40, 100), (90, 255, 200)):
        m = oracle.hsv_inrange(rgb, lo, hi)
        for filt, fm in ((ref.identity, m), (oracle.morph_open_close, oracle.morph_open_close(m))):
            for zb in (True, False):
                want = oracle.external_boxes(fm, 30, zb, max_boxes=ref.ALL_BOXES)
                got = ref.detect(oracle, rgb, [(lo, hi)], None, 30, zb, filt)
                assert len(got["masks"]) == 1 and np.array_equal(got["masks"][0], fm)
                assert got["objects"] == [b + (0,) for b in want] and got["counts"] == [len(want)]
                assert want or filt is not ref.identity          # the raw masks certainly hold boxes
                assert got["roi"] == oracle.union_box(want)
    assert ref.detect(oracle, rgb, [((200, 0, 0), (255, 255, 255))])["roi"] == oracle.union_box([])


def test_reference_classes_or_their_ranges_and_painted_planes_come_back(oracle):
    a, b = cc.BY_NAME["noise45-64x64"], cc.BY_NAME["rings_cut2-64x64"]
    rgb = ref.paint2(a, b)
    got = ref.detect(oracle, rgb, ref.TWO_RANGES, ref.TWO_CLASSES, 1, False)
    assert (a != 0).sum() and (b != 0).sum() and ((a != 0) & (b != 0)).sum()
    assert np.array_equal(got["masks"][0], a) and np.array_equal(got["masks"][1], b)
    wa, wb = oracle.external_boxes(a, 1, False, max_boxes=ref.ALL_BOXES), oracle.external_boxes(b, 1, False, max_boxes=ref.ALL_BOXES)
    assert got["objects"] == [x + (0,) for x in wa] + [x + (1,) for x in wb] and got["counts"] == [len(wa), len(wb)]
    assert got["roi"] == oracle.union_box(wa + wb)
    # red's two hue ends in one class
    rgb = cc.hsv_frame()
    hsv = oracle.rgb2hsv(rgb)
    red = ref.raw_masks(oracle, rgb, [((0, 100, 50), (9, 255, 255)), ((170, 100, 50), (179, 255, 255))], [0, 0])[0]
    h, s, v = hsv[..., 0], hsv[..., 1], hsv[..., 2]
    assert np.array_equal(red != 0, ((h <= 9) | ((h >= 170) & (h <= 179))) & (s >= 100) & (v >= 50))
    assert ((h >= 170) & (red != 0)).any() and ((h <= 9) & (red != 0)).any()


def test_host_library_exports_the_batched_objects_core():
    lib = os.path.join(ROOT, "rt-depth-map_amd", "lib", "librtdm_host.so")
    syms = subprocess.run(["nm", "-DC", lib], capture_output=True, text=True).stdout
    for name in ("rtdm::HIPObjectsCore::HIPObjectsCore(int, int, int, int, int)", "rtdm::HIPObjectsCore::setRanges",
                 "rtdm::HIPObjectsCore::detectDevice", "rtdm::HIPObjectsCore::estimateFrameClasses"):
        assert name in syms, name
