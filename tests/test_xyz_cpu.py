"""No-GPU checks of the depth map / point cloud entry points (rtdm_xyz_*, rules X1-X8 of DESIGN.md section 4.11): the symbols
are exported and declared, parameters are validated before any device use, tests/xyz_ref.py agrees with the existing depth
oracle, the OpenCV-shaped adapter compiles and the host library carries HIPXYZCore."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import xyz_ref as ref
from conftest import ROOT, load

HOST = os.path.join(ROOT, "rt-depth-map_amd", "host")
NAMES = ("rtdm_xyz_default_params rtdm_xyz_create rtdm_xyz_destroy rtdm_xyz_set_params rtdm_xyz_get_params rtdm_xyz_map "
         "rtdm_xyz_map_device rtdm_xyz_cloud rtdm_xyz_cloud_device rtdm_bm_compute_cloud").split()
QS = np.array([[1, 0, 0, -160.5], [0, 1, 0, -120.25], [0, 0, 0, 310.7], [0, 0, 1 / 2.4, 0.0]])   # test_depth_stats_device_matches_oracle


def test_symbols_are_exported_declared_and_bound():
    B = load("binding")
    L = C.CDLL(B.LIB_PATH)
    text = open(os.path.join(ROOT, "include", "rtdm.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for n in NAMES:
        assert hasattr(L, n), "librtdm_hip.so lacks " + n
        assert re.search(r"\b%s\s*\(" % n, text), "include/rtdm.h lacks " + n
        assert n in B.EXPORTS, "binding.EXPORTS lacks " + n
    for word in ("rtdm_xyz_params", "rtdm_point", "RTDM_XYZ_FIXED16 0", "RTDM_XYZ_ROUNDED 1"):
        assert word in text, word
    assert C.sizeof(B.Point) == 16 and ref.POINT.itemsize == 16
    assert B.lib().rtdm_abi_version() == 3


def test_default_params_are_the_references_call():
    B = load("binding")
    p = B.XYZParams()
    q = (C.c_double * 16)(*QS.reshape(16))
    B.lib().rtdm_xyz_default_params(C.byref(p), q, -3)
    assert list(p.Q) == list(QS.reshape(16))
    assert (p.disparity_mode, p.handle_missing_values, p.min_disparity, p.max_z) == (B.XYZ_ROUNDED, 1, -3, 1e4)


def params(B, **kw):
    p = B.XYZParams()
    B.lib().rtdm_xyz_default_params(C.byref(p), (C.c_double * 16)(*QS.reshape(16)), 0)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_validation_precedes_device_use():
    B = load("binding")
    L = B.lib()
    h = C.c_void_p()
    for bad in (dict(disparity_mode=2), dict(disparity_mode=-1), dict(handle_missing_values=2), dict(handle_missing_values=-1),
                dict(max_z=0.0), dict(max_z=-1.0), dict(max_z=float("nan"))):
        assert L.rtdm_xyz_create(C.byref(params(B, **bad)), 64, 48, 1, 0, C.byref(h)) == -1, bad
    for v in (float("nan"), float("inf"), -float("inf")):
        for i in (0, 7, 15):
            p = params(B)
            p.Q[i] = v
            assert L.rtdm_xyz_create(C.byref(p), 64, 48, 1, 0, C.byref(h)) == -1, (i, v)
    p = params(B)
    assert L.rtdm_xyz_create(None, 64, 48, 1, 0, C.byref(h)) == -7
    assert L.rtdm_xyz_create(C.byref(p), 64, 48, 1, 0, None) == -7
    assert L.rtdm_xyz_create(C.byref(p), 0, 48, 1, 0, C.byref(h)) == -2
    assert L.rtdm_xyz_create(C.byref(p), 64, 48, 0, 0, C.byref(h)) == -2
    # no row limit: only a frame whose pixel count does not fit an int is refused, and that before the device is looked for
    assert L.rtdm_xyz_create(C.byref(p), 65536, 32768, 1, 0, C.byref(h)) == -6
    import torch
    if not torch.cuda.is_available():
        assert L.rtdm_xyz_create(C.byref(p), 5000, 2, 1, 0, C.byref(h)) == -3       # wider than 4096 is served


def test_null_handles_and_planes():
    B = load("binding")
    L = B.lib()
    p = params(B)
    buf = np.zeros(64, np.int16).ctypes.data
    cnt = C.c_int()
    assert L.rtdm_xyz_set_params(None, C.byref(p)) == -7
    assert L.rtdm_xyz_get_params(None, C.byref(p)) == -7
    assert L.rtdm_xyz_map(None, buf, 16, 8, 4, buf, 96, None, 0) == -7
    assert L.rtdm_xyz_map_device(None, 1, buf, 16, 64, 8, 4, buf, 96, 384, None, 0, 0, None) == -7
    assert L.rtdm_xyz_cloud(None, buf, 16, None, 0, 0, None, 0, 8, 4, buf, 4, C.byref(cnt)) == -7
    assert L.rtdm_xyz_cloud_device(None, 1, buf, 16, 64, None, 0, 0, 0, None, 0, 0, 8, 4, buf, 64, 4, buf, None) == -7
    assert L.rtdm_bm_compute_cloud(None, None, buf, 8, buf, 8, 8, 4, None, 0, 0, None, 0, buf, 4, C.byref(cnt), None, 0) == -7
    L.rtdm_xyz_destroy(None)                     # a no-op, like the other destroy calls
    L.rtdm_xyz_default_params(None, None, 0)


def test_python_layer_raises_for_wrong_arguments():
    pkg = load()
    with pytest.raises(ValueError):
        pkg.HIPReprojector(np.eye(3), 64, 48)
    with pytest.raises(pkg.binding.RtdmError) as e:
        pkg.HIPReprojector(QS, 64, 48, mode=5)
    assert e.value.status == -1
    with pytest.raises(pkg.binding.RtdmError) as e:
        pkg.HIPReprojector(QS, 64, 48, max_z=0)
    assert e.value.status == -1


@pytest.fixture(scope="module")
def pair_disp(oracle):
    synth = load("synth")
    L, R = synth.make_pair(synth.STREAM_SEED + 78, 320, 240, 32)
    return L, oracle.bm_compute(L, R, numDisparities=32, blockSize=9)


def test_reference_agrees_with_the_depth_oracle(oracle, pair_disp):
    L, d = pair_disp
    mask = ((L > 110) * 255).astype(np.uint8)
    regions = [(40, 30, 100, 80), (0, 0, 320, 240), (317, 200, 3, 40)]
    wm, wc = oracle.depth_stats(d, QS, mask, regions)
    xyz = ref.reproject(d, QS, ref.ROUNDED, True)
    k = ref.keep(d, xyz, 0, 1e4, mask)
    for (x, y, w, h), m, c in zip(regions, wm, wc):
        kk = k[y:y + h, x:x + w]
        assert int(kk.sum()) == int(c)
        s = 0.0
        for z in xyz[y:y + h, x:x + w, 2][kk]:       # row-major, summed sequentially like the oracle
            s += float(z)
        got = (s / c) * 25.0 / 10.0 if c else 0.0
        assert got == pytest.approx(m, rel=1e-9, abs=0)
    assert [int(c) for c in wc] == [4577, 40068, 0]


def test_reference_on_the_pair_has_every_path_on_the_table(pair_disp):
    _, d = pair_disp
    assert d.shape == (240, 320)
    fixed = ref.keep(d, ref.reproject(d, QS, ref.FIXED16, True))
    rounded = ref.keep(d, ref.reproject(d, QS, ref.ROUNDED, True))
    assert int(fixed.sum()) == 55433 and int(rounded.sum()) == 55432
    q = QS.reshape(16)
    dd = ref.disparity(d, ref.FIXED16)
    x = np.arange(320.0)[None, :] * np.ones((240, 1))
    y = np.arange(240.0)[:, None] * np.ones((1, 320))
    h3 = ((q[12] * x + q[13] * y) + q[14] * dd) + q[15]
    assert int((h3 == 0).sum()) == 1362                                   # inf / NaN are produced (ROUNDED: one pixel more)
    xyz = ref.reproject(d, QS, ref.FIXED16, False)
    assert np.isinf(xyz[..., 2]).any() and not np.isfinite(xyz[..., 0][h3 == 0]).any()
    assert 0.2 < (d == -16).mean() < 0.3                                  # 26 % invalid


def test_reference_rules_on_a_hand_made_map():
    d = np.array([[-16, 0, 8, 24], [40, 41, -16, 16]], np.int16)
    assert ref.disparity(d, ref.FIXED16).tolist() == [[-1.0, 0.0, 0.5, 1.5], [2.5, 2.5625, -1.0, 1.0]]
    assert ref.disparity(d, ref.ROUNDED).tolist() == [[-1.0, 0.0, 0.0, 2.0], [2.0, 3.0, -1.0, 1.0]]      # ties to even
    Q = np.array([[1, 0, 0, -1.5], [0, 1, 0, -0.5], [0, 0, 0, 100.0], [0, 0, 0.5, 0.0]])
    xyz = ref.reproject(d, Q, ref.FIXED16, True)
    assert xyz.dtype == np.float32 and xyz.shape == (2, 4, 3)
    assert xyz[0, 0, 2] == 10000.0 and xyz[1, 2, 2] == 10000.0 and xyz[0, 0, 0] == np.float32(-1.5 / -0.5)   # X4: X untouched
    assert np.isinf(xyz[0, 1, 2]) and xyz[0, 2, 2] == np.float32(400.0)
    g = np.arange(24, dtype=np.uint8).reshape(2, 4, 3)
    pts = ref.cloud(d, Q, ref.FIXED16, True, guide=g)
    # kept: (0,2) (0,3) (1,0) (1,1) (1,3); the invalid pixels are the minimum and the d = 0 pixel is inf
    assert len(pts) == 5 and pts["z"].tolist() == [400.0, np.float32(100 / 0.75), 80.0, np.float32(100 / 1.28125), 200.0]
    assert pts["r"].tolist() == [6, 9, 12, 15, 21] and pts["b"].tolist() == [8, 11, 14, 17, 23] and set(pts["a"]) == {255}
    # without the invalid marker X4 removes valid pixels at the minimum
    d2 = np.where(d <= 0, 16, d).astype(np.int16)                        # minimum 8, at one pixel
    assert len(ref.cloud(d2, Q, ref.FIXED16, True)) == 7 and len(ref.cloud(d2, Q, ref.FIXED16, False)) == 8
    assert len(ref.cloud(d, Q, ref.FIXED16, True, mask=np.array([[1, 1, 0, 1], [0, 1, 1, 1]], np.uint8))) == 3


def test_reference_rounded_zero_is_positive():
    # ROUNDED restates an integer (CV_16S) map: raw values -8 .. -1 round to an integer zero, which is +0.0 as a double
    d = np.arange(-24, 9, dtype=np.int16).reshape(1, -1)
    r = ref.disparity(d, ref.ROUNDED)
    assert r[0, 24 - 8:24 + 9].tolist() == [0.0] * 17 and not np.signbit(r[r == 0]).any()
    assert r[0, :16].tolist() == [-2.0] + [-1.0] * 15           # -24 is a tie: to even
    Q = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 5.0], [-0.0, -0.0, 0.5, -0.0]])
    assert (ref.reproject(d, Q, ref.ROUNDED, False)[0, 16:33, 2] == np.inf).all()


SHIM = r"""
#pragma once
#include <cstddef>
namespace cv {
struct Size { int width, height; };
class Mat {
public:
    unsigned char* data; size_t step; int rows, cols;
    Mat();
    int type() const; bool empty() const; Size size() const;
};
class _InputArray { public: Mat getMat() const; };
class _OutputArray : public _InputArray { public: void create(Size sz, int type) const; };
typedef const _InputArray& InputArray;
typedef const _OutputArray& OutputArray;
}
#define CV_16SC1 3
#define CV_32FC3 21
"""


def test_xyz_adapter_compiles(tmp_path):
    (tmp_path / "opencv2").mkdir()
    (tmp_path / "opencv2" / "opencv.hpp").write_text(SHIM)
    sm = tmp_path / "stereo-matcher"
    sm.mkdir()
    (sm / "xyz-hip.h").write_text(open(os.path.join(HOST, "xyz-hip.h")).read())
    r = subprocess.run(["g++", "-std=c++11", "-Wall", "-Werror", "-fsyntax-only", "-I", str(tmp_path), "-I", HOST,
                        os.path.join(HOST, "xyz-hip.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_host_library_exports_the_xyz_core():
    lib = os.path.join(ROOT, "rt-depth-map_amd", "lib", "librtdm_host.so")
    syms = subprocess.run(["nm", "-DC", lib], capture_output=True, text=True).stdout
    for name in ("rtdm::HIPXYZCore::HIPXYZCore", "rtdm::HIPXYZCore::reprojectImageTo3D", "rtdm::HIPXYZCore::cloud",
                 "rtdm::HIPXYZCore::computeCloud"):
        assert name in syms, name
