"""No-GPU checks of the per-object depth from device lists and of the batched estimator (rtdm_depth_objects_workspace_bytes,
rtdm_depth_objects_device, rtdm_estimator_create / _destroy, rtdm_estimate_batch, rtdm_estimate_batch_device; rules D1-D6 of
DESIGN.md section 4.16): the symbols are exported, declared and bound, every refusal that needs no device is made before one is
looked for, the workspace size needs no device and grows with every argument, and a C99 caller can name the functions.

Not here: the refusals of rtdm_estimate_batch that are measured against a live estimator (pitches, strides, more classes than the
detector's max_classes).  No handle exists without a device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load

NAMES = ("rtdm_depth_objects_workspace_bytes rtdm_depth_objects_device rtdm_estimator_create rtdm_estimator_destroy "
         "rtdm_estimate_batch rtdm_estimate_batch_device").split()
NULL, BAD_PARAM, BAD_SIZE = -7, -1, -2


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
    assert "typedef struct rtdm_estimator rtdm_estimator;" in text
    assert B.lib().rtdm_abi_version() == 3 and "#define RTDM_MAX_REGIONS 64" in text
    pkg = load()
    assert callable(pkg.depth_objects_device) and callable(pkg.depth_objects_workspace_bytes)
    assert all(callable(getattr(pkg.HIPEstimator, m)) for m in ("estimate", "estimate_device", "close"))


def depth_call(L, n=2, disp=True, dpitch=64, dframe=64 * 6, W=20, H=6, Q=True, masks=True, mpitch=24, mplane=24 * 6, K=2, objects=True,
               capacity=4, counts=True, mean=True, npix=True, work=True, wbytes=None):
    """One rtdm_depth_objects_device call on device 0 whose every argument is in order unless said otherwise (the pointers are
    host memory: a call that got as far as a device would be wrong already)."""
    buf = np.zeros(1 << 16, np.uint8).ctypes.data
    q = (C.c_double * 16)()
    if wbytes is None:
        wbytes = L.rtdm_depth_objects_workspace_bytes(n, capacity, H)
    return L.rtdm_depth_objects_device(0, n, buf if disp else None, dpitch, dframe, W, H, q if Q else None, buf if masks else None, mpitch,
                                       mplane, K, buf if objects else None, capacity, buf if counts else None, 25.0,
                                       buf if mean else None, buf if npix else None, buf if work else None, wbytes, None)


def test_every_refusal_of_the_depth_call_comes_before_the_device():
    import torch
    L = load("binding").lib()
    nodev = not torch.cuda.is_available()
    if nodev:
        assert depth_call(L) == -3                                      # nothing wrong but the missing device
    for missing in ("disp", "Q", "masks", "objects", "counts", "mean", "npix", "work"):
        assert depth_call(L, **{missing: False}) == NULL, missing
    if nodev:
        assert depth_call(L, objects=False, capacity=0) == -3           # the lists are only needed with a capacity
    assert depth_call(L, n=-1, wbytes=1 << 20) == BAD_SIZE and depth_call(L, capacity=-1, wbytes=1 << 20) == BAD_SIZE
    for kw in (dict(W=0), dict(W=-3), dict(H=0), dict(H=-1)):
        assert depth_call(L, wbytes=1 << 20, **kw) == BAD_SIZE, kw
    assert depth_call(L, dpitch=65, dframe=65 * 6 + 1) == BAD_SIZE       # odd pitch
    assert depth_call(L, dframe=64 * 6 + 1) == BAD_SIZE                  # odd frame stride
    assert depth_call(L, dpitch=38, dframe=38 * 6) == BAD_SIZE           # below 2 * width
    assert depth_call(L, mpitch=19, mplane=19 * 6) == BAD_SIZE           # below width
    assert depth_call(L, dframe=64 * 6 - 2) == BAD_SIZE                  # frame 1 would begin inside frame 0
    assert depth_call(L, mplane=24 * 6 - 1) == BAD_SIZE                  # ... and plane 1 inside plane 0
    assert depth_call(L, n=1, K=2, mplane=24 * 6 - 1) == BAD_SIZE        # one frame, yet two planes
    for k in (0, -1, 9):
        assert depth_call(L, K=k) == BAD_PARAM, k
    need = L.rtdm_depth_objects_workspace_bytes(2, 4, 6)
    assert depth_call(L, wbytes=need - 1) == BAD_SIZE and depth_call(L, wbytes=0) == BAD_SIZE
    # no second frame, no second plane: the strides are free; n = 0 needs no device at all
    if nodev:
        assert depth_call(L, n=1, dframe=0) == -3 and depth_call(L, n=1, K=1, mplane=0) == -3 and depth_call(L, K=8) == -3
    assert depth_call(L, n=0) == 0


def test_workspace_size_needs_no_device_and_is_monotone():
    L = load("binding").lib()
    f = L.rtdm_depth_objects_workspace_bytes
    assert f(0, 0, 0) > 0 and f(-5, -5, -5) > 0
    base = (3, 80, 9)
    for k in range(3):
        prev = 0
        for v in (0, 1, 2, 7, 16, 17, 64, 65, 300, 4096):
            a = list(base); a[k] = v
            got = f(*a)
            assert got >= prev and got > 0, (k, v)
            prev = got
        assert prev > f(*base)                                          # ... and it does grow
    # room for the minima, a partial sum and a partial count per band of 16 rows
    assert f(3, 80, 9) >= 3 * 4 + 3 * 80 * 12 and f(3, 80, 33) >= 3 * 4 + 3 * 80 * 3 * 12


def test_estimator_create_refuses_without_a_device():
    L = load("binding").lib()
    h = C.c_void_p()
    fake = np.zeros(64, np.uint8).ctypes.data
    assert L.rtdm_estimator_create(None, None, None, 1, 1, None) == NULL
    for mb, cap in ((0, 1), (-1, 1), (1, 0), (1, -4)):
        assert L.rtdm_estimator_create(None, None, None, mb, cap, C.byref(h)) == BAD_SIZE, (mb, cap)
    for k in range(3):
        handles = [fake] * 3
        handles[k] = None
        assert L.rtdm_estimator_create(*handles, 1, 1, C.byref(h)) == NULL, k
    assert not h.value
    L.rtdm_estimator_destroy(None)                                      # as free(NULL)


@pytest.mark.parametrize("device", [False, True])
def test_refusals_of_the_batched_chain_without_an_estimator(device):
    B = load("binding")
    L = B.lib()
    buf = np.zeros(4096, np.uint8).ctypes.data
    q = (C.c_double * 16)()
    rng = (B.HsvRange * 2)(*[B.HsvRange((C.c_int * 3)(0, 150, 0), (C.c_int * 3)(9, 255, 255)) for _ in range(2)])

    def ints(*v):
        return (C.c_int * len(v))(*v)

    def call(n=1, rgb=buf, Q=q, ranges=rng, cls=ints(0, 1), nranges=2, nclasses=2, objects=buf, counts=buf, mean=buf, npix=buf):
        args = [None, n, rgb, 24, 96, buf, 24, 96, Q, ranges, cls, nranges, nclasses, 1, 1, 25.0, objects, counts, mean, npix, None, 0, 0]
        return L.rtdm_estimate_batch_device(*(args + [None])) if device else L.rtdm_estimate_batch(*args)

    assert call() == NULL                                               # nothing wrong but the handle
    for kw in (dict(rgb=None), dict(Q=None), dict(ranges=None), dict(cls=None), dict(objects=None), dict(counts=None), dict(mean=None),
               dict(npix=None)):
        assert call(**kw) == NULL, kw
    assert call(nranges=0) == BAD_PARAM and call(nranges=17) == BAD_PARAM
    assert call(nclasses=0) == BAD_PARAM and call(nclasses=9) == BAD_PARAM
    assert call(cls=ints(0, 2)) == BAD_PARAM and call(cls=ints(1, 1)) == BAD_PARAM
    assert call(n=-1) == BAD_SIZE
    assert call(n=0) == NULL                                            # n = 0 is no excuse for a missing handle


C_CALLER = r"""
#include "rtdm.h"
typedef size_t (*ws_fn)(int, int, int);
int main(void)
{
    ws_fn ws = rtdm_depth_objects_workspace_bytes;
    int (*depth)(int, int, const int16_t*, size_t, size_t, int, int, const double*, const uint8_t*, size_t, size_t, int,
                 const rtdm_object*, int, const int*, double, double*, int*, void*, size_t, void*) = rtdm_depth_objects_device;
    int (*create)(rtdm_bm*, rtdm_rectify*, rtdm_objects*, int, int, rtdm_estimator**) = rtdm_estimator_create;
    void (*destroy)(rtdm_estimator*) = rtdm_estimator_destroy;
    int (*batch)(rtdm_estimator*, int, const uint8_t*, size_t, size_t, const uint8_t*, size_t, size_t, const double*,
                 const rtdm_hsv_range*, const int*, int, int, int, int, double, rtdm_object*, int*, double*, int*, int16_t*, size_t,
                 size_t) = rtdm_estimate_batch;
    int (*batch_device)(rtdm_estimator*, int, const uint8_t*, size_t, size_t, const uint8_t*, size_t, size_t, const double*,
                        const rtdm_hsv_range*, const int*, int, int, int, int, double, rtdm_object*, int*, double*, int*, int16_t*,
                        size_t, size_t, void*) = rtdm_estimate_batch_device;
    rtdm_estimator* e = 0;
    destroy(e);
    return (ws(1, 1, 1) > 0 && depth && create && batch && batch_device) ? 0 : 1;
}
"""


def test_a_c99_caller_takes_the_addresses(tmp_path):
    src = tmp_path / "caller.c"
    src.write_text(C_CALLER)
    libdir = os.path.join(ROOT, "rt-depth-map_amd", "lib")
    exe = str(tmp_path / "caller")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-L", libdir,
                        "-lrtdm_hip", "-Wl,-rpath," + libdir, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr


def test_host_library_exports_estimate_batch():
    lib = os.path.join(ROOT, "rt-depth-map_amd", "lib", "librtdm_host.so")
    syms = subprocess.run(["nm", "-DC", lib], capture_output=True, text=True).stdout
    assert "rtdm::HIPObjectsCore::estimateBatch" in syms
