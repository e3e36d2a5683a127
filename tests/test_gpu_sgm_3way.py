"""StereoSGBM's MODE_SGBM_3WAY on the device (rtdm_sgm_set_mode, rules T1-T8 of DESIGN.md section 4.21): every result is compared
bit for bit with sgm_3way_ref.sgm_compute.  Tolerance 0.  The mode comes in through setMode on a live handle -- creating with
paths = 3 stays refused --, through the C ABI, the Python layer and the C++ core.  What the textured cases rest on (the
reference finds disparities, four stripes differ from one, T3's floor shows in the map) is asserted without a GPU in
test_sgm_3way_cpu.py.  Parity with cv::StereoSGBM itself is unpinned."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import sgm_3way_cases as cases
import sgm_3way_ref as ref
from conftest import PKG, ROOT, load

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    import torch                         # torch first: it brings its own HIP runtime and must initialise before ours
    assert torch.cuda.is_available(), "the -m gpu suite needs an MI355X"
    return load()


def assert_same(got, want, what=""):
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError("%s: %d / %d pixels differ; first at (y,x)=%s got %d want %d" % (
            what, len(bad), got.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])]))


def matcher(pkg, W, H, paths=5, cap=0, census=None, max_batch=1, **kw):
    """a handle created in another mode and set to MODE_SGBM_3WAY: the one door"""
    M = pkg.HIPSemiGlobalMatcher
    kw = dict(kw)
    kw["numOfDisparities"] = kw.pop("numDisparities")
    if census is not None:
        kw.update(cost=M.COST_CENSUS, census=census)
    m = M(width=W, height=H, preFilterCap=cap, paths=paths, max_batch=max_batch, **kw)
    try:
        m.setMode(M.MODE_SGBM_3WAY)
    except Exception:
        m.close()
        raise
    return m


def run(pkg, L, R, **kw):
    H, W = L.shape[:2]
    m = matcher(pkg, W, H, **kw)
    try:
        got = m.compute(L, R)
        assert m.path_variant == "vert3" and m.pass_stats() == (0, False)
        return got
    finally:
        m.close()


# ---- 1. the textured cases: every D class, odd W1, low frames, every window route, minD, colour, preFilterCap, census --------------
@pytest.mark.parametrize("name", [c.name for c in cases.CASES])
def test_case(pkg, name):
    c = cases.BY_NAME[name]
    L, R = c.frames()
    # the three creation modes own different buffers (paths = 4: no edge ring); the mode set on them is the same
    got = run(pkg, L, R, paths=(5, 8, 4)[len(name) % 3], cap=c.cap, census=c.census, **c.params())
    assert got.shape == (c.H, c.W)
    assert_same(got, c.want(L, R), name)


def test_every_cost_saturated_is_no_winner(pkg):
    L, R = cases.saturated_pair()
    kw = cases.saturated_params()
    want = ref.sgm_compute(L, R, **kw)
    assert (want[:, 16:] == -16).sum() > 100
    assert_same(run(pkg, L, R, **kw), want)


def test_a_frame_past_the_cost_limit_is_refused(pkg):
    r = cases.REFUSED
    L, R = cases.noise_pair(5, r["W"], r["H"])
    kw = dict(numDisparities=r["D"], blockSize=r["bs"], P2=r["P2"])
    with pytest.raises(ref.CostOverflow):
        ref.sgm_compute(L, R, **kw)
    m = matcher(pkg, r["W"], r["H"], **kw)
    try:
        with pytest.raises(pkg.binding.RtdmError) as e:
            m.compute(L, R)
        assert e.value.status == -6
        # the handle is good for the next frame
        flat = np.full((r["H"], r["W"]), 15, np.uint8)                             # (ftzero: R1's border columns cost nothing either)
        assert_same(m.compute(flat, flat), ref.sgm_compute(flat, flat, **kw))
    finally:
        m.close()


def test_a_frame_is_refused_through_a_warm_up_cost_alone(pkg, oracle):
    """T8 on a C' (k_sgm_warm3's own check): every block cost the other modes read stays below the limit"""
    r = cases.WARM_REFUSED
    L, R = cases.warm_refused_pair()
    kw = cases.warm_refused_params()
    with pytest.raises(ref.CostOverflow):
        ref.sgm_compute(L, R, **kw)
    M = pkg.HIPSemiGlobalMatcher
    m = matcher(pkg, r["W"], r["H"], **kw)
    try:
        with pytest.raises(pkg.binding.RtdmError) as e:
            m.compute(L, R)
        assert e.value.status == -6
        m.setMode(M.MODE_SGBM)                                                       # the same frame, the same handle, no C'
        got = m.compute(L, R)
        m.setMode(M.MODE_SGBM_3WAY)
        flat = np.full(L.shape, 15, np.uint8)
        assert_same(m.compute(flat, flat), ref.sgm_compute(flat, flat, **kw))        # the flag does not stick
    finally:
        m.close()
    assert_same(got, oracle.sgm_compute(L, R, paths=5, **kw), "MODE_SGBM on the pair 3WAY refuses")


# ---- 2. three frames per call, loose pitches and strides, a stream of the caller's -----------------------------------------------
def test_batch_with_loose_pitches_and_strides(pkg):
    import torch
    c = cases.BY_NAME["d64"]
    n, W, H = 3, c.W, c.H
    frames = [c.frames(seed=i) for i in range(n)]
    pitch, fstride = W + 13, (W + 13) * (H + 2)
    dpitch, dstride = (W + 5) * 2, (W + 5) * 2 * (H + 1)
    hL = np.full((n, fstride), 77, np.uint8); hR = np.full((n, fstride), 99, np.uint8)
    for i, (L, R) in enumerate(frames):
        hL[i, :pitch * H].reshape(H, pitch)[:, :W] = L
        hR[i, :pitch * H].reshape(H, pitch)[:, :W] = R
    m = matcher(pkg, W, H, max_batch=2, cap=c.cap, **c.params())                    # two chunks: 2 + 1 frames
    try:
        dL, dR = torch.from_numpy(hL).cuda(), torch.from_numpy(hR).cuda()
        dD = torch.full((n, dstride // 2), -999, dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        B = pkg.binding
        with torch.cuda.stream(s):
            B.check(B.lib().rtdm_sgm_compute_device_cn(m._h, 1, n, dL.data_ptr(), dR.data_ptr(), pitch, fstride, W, H, dD.data_ptr(),
                                                       dpitch, dstride, s.cuda_stream), "rtdm_sgm_compute_device_cn")
        s.synchronize()
        assert m.path_variant == "vert3" and m.pass_stats() == (0, False)
        out = dD.cpu().numpy()
    finally:
        m.close()
    for i, (L, R) in enumerate(frames):
        plane = out[i, :(dpitch // 2) * H].reshape(H, dpitch // 2)
        assert_same(plane[:, :W], c.want(L, R), "frame %d" % i)
        assert (plane[:, W:] == -999).all() and (out[i, (dpitch // 2) * H:] == -999).all()      # nothing outside the rows
    assert len({out[i].tobytes() for i in range(n)}) == n


# ---- 3. setMode on a live handle: the order of calls, and nothing existing changed -------------------------------------------------
def test_set_mode_back_and_forth(pkg, oracle):
    c = cases.BY_NAME["d16_odd_w1"]
    L, R = c.frames()
    M = pkg.HIPSemiGlobalMatcher
    m = M(numOfDisparities=c.D, blockSize=c.bs, width=c.W, height=c.H, paths=5, speckleWindowSize=0)
    try:
        first = m.compute(L, R)
        v1, s1 = m.path_variant, m.pass_stats()
        m.setMode(M.MODE_SGBM_3WAY)
        assert (m.mode, m.params.paths, m.getMode()) == (M.MODE_SGBM_3WAY, 3, 2)
        mid = m.compute(L, R)
        assert m.path_variant == "vert3" and m.pass_stats() == s1                     # the pass statistics do not move
        m.setMode(M.MODE_SGBM)
        assert (m.mode, m.params.paths) == (M.MODE_SGBM, 5)
        last = m.compute(L, R)
        assert m.path_variant == v1 == "sweep" and m.pass_stats()[0] == 2 * s1[0]
        # every mode on the one handle, each against its own reference
        m.setMode(M.MODE_HH)
        hh = m.compute(L, R)
        m.setMode(M.MODE_HH4)
        h4 = m.compute(L, R)
        assert m.path_variant == "vert"
        with pytest.raises(pkg.binding.RtdmError) as e:
            pkg.binding.check(pkg.binding.lib().rtdm_sgm_set_mode(m._h, 4), "rtdm_sgm_set_mode")
        assert e.value.status == -1 and m.getMode() == M.MODE_HH4                     # a refused call leaves the mode
    finally:
        m.close()
    kw = dict(numDisparities=c.D, blockSize=c.bs, speckleWindowSize=0)
    assert first.tobytes() == last.tobytes()
    assert_same(first, oracle.sgm_compute(L, R, paths=5, **kw), "MODE_SGBM")
    assert_same(mid, ref.sgm_compute(L, R, **kw), "MODE_SGBM_3WAY")
    assert_same(hh, oracle.sgm_compute(L, R, paths=8, **kw), "MODE_HH")
    import sgm_hh4_ref
    assert_same(h4, sgm_hh4_ref.sgm_compute(L, R, **kw), "MODE_HH4")
    assert (mid != first).any()


def test_a_handle_created_without_a_ring_runs_the_sweep_modes_as_half(pkg, oracle):
    c = cases.BY_NAME["minD_p4"]
    L, R = c.frames()
    M = pkg.HIPSemiGlobalMatcher
    m = M(numOfDisparities=c.D, blockSize=c.bs, minDisparity=c.minD, width=c.W, height=c.H, paths=4)
    try:
        m.setMode(M.MODE_SGBM)
        got = m.compute(L, R)
        assert m.path_variant == "half" and m.pass_stats() == (0, False)
    finally:
        m.close()
    assert_same(got, oracle.sgm_compute(L, R, numDisparities=c.D, blockSize=c.bs, minDisparity=c.minD, paths=5))


def test_wide_handles_refuse_the_mode(pkg):
    M = pkg.HIPSemiGlobalMatcher
    m = M(numOfDisparities=272, width=320, height=8, paths=5)
    try:
        with pytest.raises(pkg.binding.RtdmError) as e:
            m.setMode(M.MODE_SGBM_3WAY)
        assert e.value.status == -6 and m.mode == M.MODE_SGBM and m.getMode() == M.MODE_SGBM
        m.setMode(M.MODE_HH4)                                                        # the other modes plan as ever
        assert m.mode == M.MODE_HH4
    finally:
        m.close()
    for shut in (dict(mode=M.MODE_SGBM_3WAY), dict(paths=3)):                        # the creation door
        with pytest.raises(pkg.binding.RtdmError) as e:
            M(numOfDisparities=16, width=64, height=16, **shut)
        assert e.value.status == -6


def test_right_matcher_copies_the_mode(pkg):
    c = cases.BY_NAME["minD_m8"]
    L, R = c.frames()
    left = matcher(pkg, c.W, c.H, **c.params())
    right = pkg.create_right_matcher(left)
    try:
        assert right.mode == right.MODE_SGBM_3WAY and right.getMode() == 2
        got = right.compute(R, L)
        assert right.path_variant == "vert3"
        p = right.params
        want = ref.sgm_compute(R, L, numDisparities=p.numDisparities, minDisparity=p.minDisparity, blockSize=p.blockSize, P1=p.P1,
                               P2=p.P2, uniquenessRatio=p.uniquenessRatio, speckleWindowSize=p.speckleWindowSize,
                               speckleRange=p.speckleRange)
        assert_same(got, want)
    finally:
        right.close(); left.close()


# ---- 4. RTDM_SGM_DUAL=0 (read once per process: a child) and the debug switch that is ignored --------------------------------------
CHILD = r"""
import importlib, os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import numpy as np
import torch
assert torch.cuda.is_available()
pkg = importlib.import_module("rt-depth-map_amd")
import sgm_3way_cases as cases
import test_gpu_sgm_3way as T
out = {}
for name in T.DUAL_CASES:
    c = cases.BY_NAME[name]
    L, R = c.frames()
    out[name] = T.run(pkg, L, R, cap=c.cap, census=c.census, **c.params())
np.savez(sys.argv[2], **out)
"""
DUAL_CASES = ("d16_odd_w1", "d128", "d256")


def test_horizontal_passes_one_after_the_other_in_a_child_process(pkg, tmp_path):
    script = tmp_path / "child.py"
    script.write_text(CHILD)
    out = tmp_path / "dual.npz"
    r = subprocess.run([sys.executable, str(script), ROOT, str(out)], env=dict(os.environ, RTDM_SGM_DUAL="0", RTDM_SGM_SWEEP="0"),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    z = np.load(out)
    for name in DUAL_CASES:
        c = cases.BY_NAME[name]
        assert_same(z[name], c.want(*c.frames()), name)


def test_forced_wide_paths_are_ignored(pkg):
    c = cases.BY_NAME["d48_dead_lanes"]
    L, R = c.frames()
    pkg.binding.lib().rtdm_debug_sgm_wide_paths(1)
    try:
        got = run(pkg, L, R, **c.params())                                           # (run asserts "vert3")
    finally:
        pkg.binding.lib().rtdm_debug_sgm_wide_paths(0)
    assert_same(got, c.want(L, R))


# ---- 5. the C++ core ---------------------------------------------------------------------------------------------------------------
def test_host_core_set_mode(pkg, tmp_path):
    c = cases.BY_NAME["d16_odd_w1"]
    L, R = c.frames()
    src = tmp_path / "t.cpp"
    src.write_text(r"""
#include "hip_matcher_core.h"
#include <cstdio>
#include <vector>
int main(int argc, char** argv) {
    const int W = %d, H = %d;
    std::vector<unsigned char> l(W * H), r(W * H);
    std::vector<short> d(W * H);
    FILE* f = std::fopen(argv[1], "rb");
    if (!f || std::fread(l.data(), 1, l.size(), f) != l.size() || std::fread(r.data(), 1, r.size(), f) != r.size()) return 3;
    std::fclose(f);
    rtdm::HIPSGMCore a(%d, 0, %d, 10, 0, 32, 1, W, H, 0, 5);
    const int bad = a.setMode(7), ok = a.setMode(rtdm::MODE_SGBM_3WAY);
    const int rc = a.compute(l.data(), W, r.data(), W, H, W, d.data(), W * 2);
    rtdm::HIPSGMCore* rm = rtdm::createRightMatcher(a);
    std::printf("status=%%d bad=%%d ok=%%d mode=%%d paths=%%d created=%%d rc=%%d right=%%d/%%d/%%d\n", a.status(), bad, ok, a.mode(), a.params().paths,
                a.createdPaths(), rc, rm->mode(), rm->params().paths, rm->createdPaths());
    delete rm;
    f = std::fopen(argv[2], "wb");
    std::fwrite(d.data(), 2, d.size(), f);
    std::fclose(f);
    return 0;
}
""" % (c.W, c.H, c.bs, c.D))
    libdir = os.path.join(ROOT, PKG, "lib")
    exe = tmp_path / "t"
    subprocess.check_call(["g++", "-std=c++11", "-I", os.path.join(ROOT, PKG, "host"), "-I", os.path.join(ROOT, "include"), str(src),
                           "-o", str(exe), "-L", libdir, "-lrtdm_host", "-lrtdm_hip", "-Wl,-rpath," + libdir])
    (tmp_path / "in.bin").write_bytes(L.tobytes() + R.tobytes())
    out = subprocess.run([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "status=0 bad=-1 ok=0 mode=2 paths=3 created=5 rc=0 right=2/3/5" in out.stdout, out.stdout
    got = np.frombuffer((tmp_path / "out.bin").read_bytes(), np.int16).reshape(c.H, c.W)
    assert_same(got, c.want(L, R), "HIPSGMCore::setMode")
