"""StereoSGBM's MODE_HH4 (paths = 4, rule R4') on the CPU side: the NumPy R4 of sgm_hh4_ref.py against the C oracle's recurrence
for the direction sets the oracle has (5 and 8), the parameter checks of rtdm_sgm_create without a device, the Python mode=
mapping, and the C++ adapter's new constructor argument.  The GPU tests (test_gpu_sgm_hh4.py) compare the device against
sgm_hh4_ref bit for bit."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import sgm_cn_ref
import sgm_hh4_ref as ref
from conftest import ROOT, load
from test_wls_adapter import MATCHER, SHIM

HOST = os.path.join(ROOT, "rt-depth-map_amd", "host")

# W, H, D, minD, blockSize, P1, P2, uniquenessRatio
CASES = [(160, 60, 32, 0, 5, 600, 2400, 10), (131, 37, 16, -5, 3, 8, 32, 0), (200, 48, 64, 3, 7, 600, 32000, 15)]


def _anchor(oracle, Cc, P1, P2, W, H, p):
    """the 5 / 8 sets equal orc_sgm_aggregate_paths byte for byte; the 4-set map differs from both somewhere"""
    maps = {}
    for paths in (5, 8):
        S = np.zeros_like(Cc)
        oracle.lib().orc_sgm_aggregate_paths(ref._p(Cc, C.c_uint16), Cc.shape[1], Cc.shape[0], Cc.shape[2], P1, P2, paths,
                                            ref._p(S, C.c_uint16))
        mine = ref.aggregate(Cc, P1, P2, ref.DIRS[paths])
        assert mine.tobytes() == S.tobytes(), "paths %d" % paths
        maps[paths] = ref.finish(S, W, H, p)
    S4 = ref.aggregate(Cc, P1, P2, ref.DIRS[4])
    d4 = ref.finish(S4, W, H, p)
    assert (d4 != maps[5]).any() and (d4 != maps[8]).any()
    assert (d4 != (p.minDisparity - 1) * 16).any()
    return S4


@pytest.mark.parametrize("W,H,D,minD,bs,P1,P2,uniq", CASES)
def test_numpy_r4_equals_oracle_on_its_direction_sets(oracle, synth, W, H, D, minD, bs, P1, P2, uniq):
    L, R = synth.make_pair(synth.STREAM_SEED + 77, W, H, D)
    p = oracle.make_sgm_params(blockSize=bs, minDisparity=minD, numDisparities=D, P1=P1, P2=P2, uniquenessRatio=uniq, paths=4)
    Cc, _ = ref.block_costs(L, R, p)
    S4 = _anchor(oracle, Cc, P1, P2, W, H, p)
    if P2 == 32000:
        assert (S4 == 32767).mean() > 0.5              # the saturating sum (R5) is exercised, not only present


def test_numpy_r4_equals_oracle_on_a_colour_pair(oracle):
    rng = np.random.default_rng(12)
    W, H, D, minD = 90, 22, 16, -3
    T = rng.integers(0, 256, (H, W + 7, 3)).astype(np.float64)
    T = ((T + np.roll(T, 1, 1) + np.roll(T, 1, 0)) / 3).astype(np.uint8)
    L, R = T[:, 7:].copy(), T[:, :W].copy()
    p = oracle.make_sgm_params(blockSize=3, minDisparity=minD, numDisparities=D, paths=4)
    Cc, cmax = ref.block_costs(L, R, p, preFilterCap=31)
    assert cmax > 0
    _anchor(oracle, Cc, 600, 2400, W, H, p)


def test_chain_equals_oracle_compute_for_its_modes(oracle, synth):
    # sgm_compute with the oracle's own direction sets is orc_sgm_compute (early return and refusal included)
    L, R = synth.make_pair(synth.STREAM_SEED + 78, 120, 30, 32)
    for paths in (5, 8):
        kw = dict(numDisparities=32, minDisparity=-4, blockSize=5, paths=paths)
        assert np.array_equal(ref.sgm_compute(L, R, **kw), oracle.sgm_compute(L, R, **kw))
    got = ref.sgm_compute(L[:, :30].copy(), R[:, :30].copy(), numDisparities=48)
    assert (got == -16).all()                                                    # W1 <= 0
    rng = np.random.default_rng(1)
    Ln, Rn = ((rng.integers(0, 2, (2, 30, 80)) * 255).astype(np.uint8))
    with pytest.raises(ref.CostOverflow):
        ref.sgm_compute(Ln, Rn, numDisparities=16, blockSize=31, P2=2400, speckleWindowSize=0)
    with pytest.raises(ValueError):
        oracle.sgm_compute(Ln, Rn, numDisparities=16, blockSize=31, P2=2400, speckleWindowSize=0, paths=8)
    assert sgm_cn_ref.CostOverflow is ref.CostOverflow


def test_create_checks_paths_before_the_device():
    import torch
    B = load("binding")
    L = B.lib()
    h = C.c_void_p()

    def create(paths):
        p = B.SGMParams(5, 0, 64, 600, 2400, 10, 100, 32, 1, paths)
        rc = L.rtdm_sgm_create(C.byref(p), 128, 32, 1, 0, C.byref(h))
        if rc == 0:
            L.rtdm_sgm_destroy(h)
        return rc
    for paths in (0, 1, 2, 6, 7, 9):
        assert create(paths) == -1, paths
    assert create(3) == -6                               # MODE_SGBM_3WAY: valid for the library, not implemented
    assert create(4) != -1                               # MODE_HH4 is served
    sp = B.SGMParams(7, -8, 48, 600, 2400, 10, 100, 32, 1, 4)
    rs = B.SGMParams()
    assert L.rtdm_sgm_right_params(C.byref(sp), C.byref(rs)) == 0
    assert (rs.paths, rs.minDisparity, rs.numDisparities, rs.blockSize) == (4, -(-8 + 48) + 1, 48, 7)
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    assert create(4) == -3
    assert create(5) == -3 and create(8) == -3


def test_python_mode_keyword_maps_to_paths():
    import torch
    pkg = load()
    M = pkg.HIPSemiGlobalMatcher
    assert (M.MODE_SGBM, M.MODE_HH, M.MODE_SGBM_3WAY, M.MODE_HH4) == (0, 1, 2, 3)
    kw = dict(numOfDisparities=16, width=64, height=16)
    # the checks that need no device
    for mode, paths in ((M.MODE_HH4, 8), (M.MODE_HH4, 5), (M.MODE_SGBM, 4), (M.MODE_HH, 5)):
        with pytest.raises(ValueError):
            M(mode=mode, paths=paths, **kw)
    with pytest.raises(ValueError):
        M(mode=7, **kw)
    with pytest.raises(pkg.binding.RtdmError) as e:
        M(mode=M.MODE_SGBM_3WAY, **kw)
    assert e.value.status == -6
    with pytest.raises(pkg.binding.RtdmError) as e:
        M(paths=3, **kw)
    assert e.value.status == -6
    if torch.cuda.is_available():
        for args, paths in ((dict(mode=M.MODE_SGBM), 5), (dict(mode=M.MODE_HH), 8), (dict(mode=M.MODE_HH4), 4),
                            (dict(paths=4), 4), (dict(mode=M.MODE_HH4, paths=4), 4), (dict(), 8)):
            m = M(**dict(kw, **args))
            try:
                assert m.params.paths == paths and M._MODE_PATHS[m.mode] == paths
            finally:
                m.close()
    else:
        # without a device the mapping shows in what the library is asked for: accepted parameters reach the device check
        for args in (dict(mode=M.MODE_SGBM), dict(mode=M.MODE_HH), dict(mode=M.MODE_HH4), dict(paths=4),
                     dict(mode=M.MODE_HH4, paths=4)):
            with pytest.raises(pkg.binding.RtdmError) as e:
                M(**dict(kw, **args))
            assert e.value.status == -3, args


def test_adapter_compiles_with_and_without_the_mode_argument(tmp_path):
    """the nine-argument reference constructor still compiles unchanged; a tenth argument selects the mode"""
    (tmp_path / "opencv2").mkdir()
    (tmp_path / "opencv2" / "opencv.hpp").write_text(SHIM)
    sm = tmp_path / "stereo-matcher"
    sm.mkdir()
    (sm / "stereo-matcher.h").write_text(MATCHER)
    (sm / "sgbm-hip.h").write_text(open(os.path.join(HOST, "sgbm-hip.h")).read())
    user = tmp_path / "user.cpp"
    user.write_text(r"""
#include "stereo-matcher/sgbm-hip.h"
BlockMatcher* nine() { return new HIPSemiGlobalMatcher(5, 0, 128, 10, 100, 32, 1, 1280, 720); }
BlockMatcher* hh4() { return new HIPSemiGlobalMatcher(5, 0, 128, 10, 100, 32, 1, 1280, 720, rtdm::MODE_HH4); }
static_assert(rtdm::MODE_SGBM == 0 && rtdm::MODE_HH == 1 && rtdm::MODE_SGBM_3WAY == 2 && rtdm::MODE_HH4 == 3, "cv's values");
int paths[] = { rtdm::HIPSGMCore::pathsForMode(rtdm::MODE_SGBM), rtdm::HIPSGMCore::pathsForMode(rtdm::MODE_HH),
                rtdm::HIPSGMCore::pathsForMode(rtdm::MODE_SGBM_3WAY), rtdm::HIPSGMCore::pathsForMode(rtdm::MODE_HH4) };
""")
    for src in (str(user), os.path.join(HOST, "sgbm-hip.cpp")):
        r = subprocess.run(["g++", "-std=c++11", "-Wall", "-Werror", "-fsyntax-only", "-I", str(tmp_path), "-I", HOST,
                            "-I", os.path.join(ROOT, "include"), src], capture_output=True, text=True)
        assert r.returncode == 0, src + "\n" + r.stderr


def test_host_core_maps_modes_to_paths(tmp_path):
    """pathsForMode at run time, and a core created with paths = 4 fails for the device's absence, not for its parameters"""
    import torch
    src = tmp_path / "t.cpp"
    src.write_text(r"""
#include "hip_matcher_core.h"
#include <cstdio>
int main() {
    using rtdm::HIPSGMCore;
    if (HIPSGMCore::pathsForMode(0) != 5 || HIPSGMCore::pathsForMode(1) != 8 || HIPSGMCore::pathsForMode(2) != 3 ||
        HIPSGMCore::pathsForMode(3) != 4 || HIPSGMCore::pathsForMode(9) != 0) return 2;
    HIPSGMCore a(5, 0, 64, 10, 100, 32, 1, 128, 32, 0, HIPSGMCore::pathsForMode(rtdm::MODE_HH4));
    HIPSGMCore b(5, 0, 64, 10, 100, 32, 1, 128, 32, 0, HIPSGMCore::pathsForMode(rtdm::MODE_SGBM_3WAY));
    HIPSGMCore c(5, 0, 64, 10, 100, 32, 1, 128, 32, 0, HIPSGMCore::pathsForMode(42));
    std::printf("hh4=%d 3way=%d bad=%d\n", a.status(), b.status(), c.status());
    return 0;
}
""")
    libdir = os.path.join(ROOT, "rt-depth-map_amd", "lib")
    exe = tmp_path / "t"
    subprocess.check_call(["g++", "-std=c++11", "-I", HOST, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", libdir, "-lrtdm_host", "-lrtdm_hip", "-Wl,-rpath," + libdir])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    want_hh4 = "hh4=0" if torch.cuda.is_available() else "hh4=-3"
    assert want_hh4 in out.stdout and "3way=-6" in out.stdout and "bad=-1" in out.stdout, out.stdout
