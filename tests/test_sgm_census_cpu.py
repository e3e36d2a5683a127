"""StereoSGBM's census pixel cost (rtdm_sgm_set_cost, rules N1-N5 of DESIGN.md section 4.20) on the CPU side: the NumPy reference
sgm_census_ref.py against a literal restatement of N1 and against the properties N1 / N2 promise, the C ABI's and the Python
layer's argument checks without a device, the C++ adapter, and that the inputs of the GPU tests (sgm_census_cases.py) do what
they are built for.  The GPU tests (test_gpu_sgm_census.py) compare the device against sgm_census_ref bit for bit."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import sgm_census_cases as cases
import sgm_census_ref as ref
import sgm_cn_ref
from conftest import ROOT, load
from test_wls_adapter import MATCHER, SHIM

HOST = os.path.join(ROOT, "rt-depth-map_amd", "host")


def literal_descriptors(img, cw, ch):
    """N1 word for word: a loop over pixels and offsets -> a set of the offsets whose bit is set, per pixel"""
    H, W = img.shape
    out = {}
    for y in range(H):
        for x in range(W):
            bits = set()
            for j in range(-(ch // 2), ch // 2 + 1):
                for i in range(-(cw // 2), cw // 2 + 1):
                    if (i, j) == (0, 0):
                        continue
                    if img[min(max(y + j, 0), H - 1)][min(max(x + i, 0), W - 1)] < img[y][x]:
                        bits.add((i, j))
            out[(y, x)] = bits
    return out


@pytest.mark.parametrize("cw,ch", cases.WINDOWS)
def test_vectorised_descriptor_equals_the_literal_loop(cw, ch):
    img = np.random.default_rng(100 * cw + ch).integers(0, 4, (9, 12)).astype(np.uint8)       # 12 x 9, many ties
    got = ref.descriptors(img, cw, ch)
    want = literal_descriptors(img, cw, ch)
    offs = ref.offsets(cw, ch)
    assert len(offs) == cw * ch - 1 <= 62 and len(set(offs)) == len(offs) and (0, 0) not in offs
    nset = 0
    for (y, x), bits in want.items():
        word = int(got[y, x])
        assert word >> len(offs) == 0
        assert {offs[k] for k in range(len(offs)) if word >> k & 1} == bits, (y, x)
        nset += len(bits)
    assert 0 < nset < img.size * len(offs)                 # ties and strict comparisons both occur


@pytest.mark.parametrize("cw,ch", cases.WINDOWS)
def test_costs_are_bounded_and_zero_for_a_pixel_against_itself(cw, ch):
    rng = np.random.default_rng(7 + cw * ch)
    W, H, D = 41, 11, 16
    L, R = rng.integers(0, 256, (2, H, W)).astype(np.uint8)
    M = cw * ch - 1
    for minD in (0, -5, 3):
        pix = ref.pixel_cost(L, R, minD, D, cw, ch)
        assert pix.shape == (H, (W + min(minD, 0)) - max(minD + D, 0), D) and pix.dtype == np.uint16
        assert pix.max() <= M and pix.max() > M // 2                     # noise: about half the bits differ somewhere
    # identical images: cost 0 at the disparity that pairs every pixel with itself
    same = ref.pixel_cost(L, L, -3, D, cw, ch)
    assert (same[:, :, 3] == 0).all() and (same[:, :, 4] != 0).any()
    # a view moved by s columns: cost 0 at d = s wherever both windows lie inside the frames
    s, hw = 6, cw // 2
    T = rng.integers(0, 256, (H, W + s)).astype(np.uint8)
    mv = ref.pixel_cost(T[:, :W].copy(), T[:, s:].copy(), 0, D, cw, ch)      # left[x] = right[x - s]
    inner = slice(hw, W - D - hw - s)                                            # domain columns x - 16 with x - s - hw >= 0, x + hw + s < W
    assert (mv[:, inner, s] == 0).all() and (mv[:, inner, s + 1] != 0).any()


@pytest.mark.parametrize("cw,ch", cases.WINDOWS)
def test_descriptors_do_not_change_under_an_increasing_mapping(cw, ch):
    img = np.random.default_rng(31 * cw + ch).integers(0, 121, (14, 23)).astype(np.uint8)
    img[3:6, 4:9] = 57                                                            # a plateau: ties stay ties
    mapped = (2 * img.astype(np.int64) + 10).astype(np.uint8)
    assert mapped.max() <= 250 and (mapped != img).all()
    assert np.array_equal(ref.descriptors(img, cw, ch), ref.descriptors(mapped, cw, ch))
    # (a mapping that is not increasing does change them)
    assert not np.array_equal(ref.descriptors(img, cw, ch), ref.descriptors((255 - img).astype(np.uint8), cw, ch))


def test_popcount64():
    a = np.array([0, 1, 0xffffffffffffffff, 0x8000000000000001, 0x3fffffffffffffff], np.uint64)
    assert ref.popcount64(a).tolist() == [0, 1, 64, 2, 62]


def test_header_and_exports_carry_both_functions():
    B = load("binding")
    text = open(os.path.join(ROOT, "include", "rtdm.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+rtdm_sgm_set_cost\s*\(\s*rtdm_sgm\s*\*\s*sg\s*,\s*int\s+cost\s*,\s*int\s+census_width\s*,\s*int\s+census_height\s*\)\s*;", code)
    assert re.search(r"\bint\s+rtdm_sgm_get_cost\s*\(\s*const\s+rtdm_sgm\s*\*\s*sg\s*,\s*int\s*\*\s*cost\s*,\s*int\s*\*\s*census_width\s*,\s*"
                     r"int\s*\*\s*census_height\s*\)\s*;", code)
    assert re.search(r"#define\s+RTDM_SGM_COST_BT\s+0\b", code) and re.search(r"#define\s+RTDM_SGM_COST_CENSUS\s+1\b", code)
    assert "rtdm_sgm_set_cost" in B.EXPORTS and "rtdm_sgm_get_cost" in B.EXPORTS
    assert (B.SGM_COST_BT, B.SGM_COST_CENSUS) == (0, 1)
    L = C.CDLL(B.LIB_PATH)
    assert hasattr(L, "rtdm_sgm_set_cost") and hasattr(L, "rtdm_sgm_get_cost")
    # the structure and the ABI version are what they were
    assert C.sizeof(B.SGMParams) == 40 and B.lib().rtdm_abi_version() == 3
    # N1-N5 and the absence of a library counterpart are stated where a caller reads
    for name in ("N1", "N2", "N3", "N4", "N5"):
        assert re.search(r"\b%s\b" % name, text), name
    assert "NO counterpart" in text and "unmeasured" in text


def test_null_handle_is_refused():
    L = load("binding").lib()
    c = C.c_int(5)
    assert L.rtdm_sgm_set_cost(None, 1, 9, 7) == -7
    assert L.rtdm_sgm_set_cost(None, 0, 0, 0) == -7
    assert L.rtdm_sgm_set_cost(None, 9, 9, 7) == -7                               # NULL is found first
    assert L.rtdm_sgm_get_cost(None, C.byref(c), None, None) == -7 and c.value == 5
    assert L.rtdm_sgm_get_cost(None, None, None, None) == -7


def test_python_keywords_are_checked_before_the_device():
    import torch
    pkg = load()
    M = pkg.HIPSemiGlobalMatcher
    assert (M.COST_BT, M.COST_CENSUS) == (0, 1)
    kw = dict(numOfDisparities=16, width=64, height=16)
    for bad in (dict(cost=2), dict(cost=-1), dict(cost="census"), dict(cost=None), dict(cost=True),
                dict(cost=M.COST_CENSUS, census=(4, 7)), dict(cost=M.COST_CENSUS, census=(11, 7)),
                dict(cost=M.COST_CENSUS, census=(9, 9)), dict(cost=M.COST_CENSUS, census=(9, 1)),
                dict(cost=M.COST_CENSUS, census=(7, 9)), dict(cost=M.COST_CENSUS, census=9),
                dict(cost=M.COST_CENSUS, census=(9, 7, 5)), dict(cost=M.COST_CENSUS, census=(9.0, 7)),
                dict(cost=M.COST_CENSUS, census=None), dict(cost=M.COST_BT, census="ab")):
        with pytest.raises(ValueError):
            M(**dict(kw, **bad))
    # the same checks without a handle
    assert M._check_cost(M.COST_CENSUS, (np.int64(5), 3)) == (1, (5, 3))
    assert M._check_cost(M.COST_BT, (4, 4)) == (0, (4, 4))                        # BT ignores the sizes
    if torch.cuda.is_available():
        m = M(cost=M.COST_CENSUS, census=(5, 3), **kw)
        try:
            assert m.getCost() == (M.COST_CENSUS, (5, 3))
        finally:
            m.close()
    else:
        for good in (dict(), dict(cost=M.COST_BT), dict(cost=M.COST_CENSUS), dict(cost=M.COST_CENSUS, census=(3, 3)),
                     dict(cost=M.COST_CENSUS, census=[9, 7]), dict(cost=M.COST_BT, census=(4, 4))):
            with pytest.raises(pkg.binding.RtdmError) as e:
                M(**dict(kw, **good))
            assert e.value.status == -3, good


def test_adapter_with_set_cost_compiles(tmp_path):
    """sgbm-hip.h with setCost, in the reference's dialect"""
    (tmp_path / "opencv2").mkdir()
    (tmp_path / "opencv2" / "opencv.hpp").write_text(SHIM)
    sm = tmp_path / "stereo-matcher"
    sm.mkdir()
    (sm / "stereo-matcher.h").write_text(MATCHER)
    (sm / "sgbm-hip.h").write_text(open(os.path.join(HOST, "sgbm-hip.h")).read())
    user = tmp_path / "user.cpp"
    user.write_text(r"""
#include "stereo-matcher/sgbm-hip.h"
int census(HIPSemiGlobalMatcher& m) { return m.setCost(RTDM_SGM_COST_CENSUS); }
int census53(HIPSemiGlobalMatcher& m) { return m.setCost(RTDM_SGM_COST_CENSUS, 5, 3); }
int back(HIPSemiGlobalMatcher& m) { return m.setCost(RTDM_SGM_COST_BT); }
int read(HIPSemiGlobalMatcher& m) { return m.getCore()->cost() * 100 + m.getCore()->censusWidth() * 10 + m.getCore()->censusHeight(); }
static_assert(RTDM_SGM_COST_BT == 0 && RTDM_SGM_COST_CENSUS == 1, "the header's values");
""")
    for src in (str(user), os.path.join(HOST, "sgbm-hip.cpp")):
        r = subprocess.run(["g++", "-std=c++11", "-Wall", "-Werror", "-fsyntax-only", "-I", str(tmp_path), "-I", HOST,
                            "-I", os.path.join(ROOT, "include"), src], capture_output=True, text=True)
        assert r.returncode == 0, src + "\n" + r.stderr


def test_host_core_set_cost_without_a_device(tmp_path):
    """a core without a handle answers setCost with its status; the getters keep the defaults"""
    import torch
    src = tmp_path / "t.cpp"
    src.write_text(r"""
#include "hip_matcher_core.h"
#include <cstdio>
int main() {
    rtdm::HIPSGMCore a(5, 0, 64, 10, 100, 32, 1, 128, 32, 0, 5);
    const int bad = a.setCost(7), badw = a.setCost(RTDM_SGM_COST_CENSUS, 4, 7), ok = a.setCost(RTDM_SGM_COST_CENSUS, 5, 3);
    std::printf("status=%d bad=%d badw=%d ok=%d cost=%d %dx%d\n", a.status(), bad, badw, ok, a.cost(), a.censusWidth(), a.censusHeight());
    rtdm::HIPSGMCore* r = rtdm::createRightMatcher(a);
    std::printf("right cost=%d %dx%d\n", r->cost(), r->censusWidth(), r->censusHeight());
    delete r;
    return 0;
}
""")
    libdir = os.path.join(ROOT, "rt-depth-map_amd", "lib")
    exe = tmp_path / "t"
    subprocess.check_call(["g++", "-std=c++11", "-I", HOST, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", libdir, "-lrtdm_host", "-lrtdm_hip", "-Wl,-rpath," + libdir])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    if torch.cuda.is_available():
        assert "status=0 bad=-1 badw=-1 ok=0 cost=1 5x3" in out.stdout and "right cost=1 5x3" in out.stdout, out.stdout
    else:
        assert "status=-3 bad=-3 badw=-3 ok=-3 cost=0 9x7" in out.stdout and "right cost=0 9x7" in out.stdout, out.stdout


# ---- the GPU tests' inputs, checked where no GPU is needed ------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(cases.ROUTES)), ids=[cases.case_id(c) for c in cases.ROUTES])
def test_route_cases_find_their_disparity(oracle, i):
    """every textured case of test_gpu_sgm_census.py: at least 30 % of the reference's domain pixels are valid, most of them at the
    disparity the pair was built with, and the pair is not refused (the checked route, 62 * 441 + 8000 > 32767, included)"""
    c = cases.ROUTES[i]
    W, H, D, minD, bs, paths, census, n, P2 = c
    Ls, Rs = cases.case_frames(i, c)
    assert Ls.shape == (n, H, W) and (W + min(minD, 0)) - max(minD + D, 0) > 0
    for f in range(n):
        want = ref.sgm_compute(Ls[f], Rs[f], census=census, **cases.params(c))         # raises CostOverflow if refused
        share = cases.valid_share(want, c)
        assert share >= 0.30, "frame %d: %.3f" % (f, share)
        x0, x1 = max(minD + D, 0), W + min(minD, 0)
        dom = want[:, x0:x1]
        assert (np.abs(dom[dom != (minD - 1) * 16] - 16 * (minD + 3 + 2 * f)) <= 8).mean() > 0.8
    if bs == 21:
        M = census[0] * census[1] - 1
        assert M * bs * bs + P2 > 32767                                                 # the device checks this frame's block costs
        _, cmax = ref.block_costs(Ls[0], Rs[0], oracle.make_sgm_params(**cases.params(c)), census)
        assert cmax <= 32767 - P2


def test_refusal_and_invariance_inputs(oracle):
    # the refusal pair is refused by the reference, the constant pair after it is not
    L, R = cases.noise_pair(9200, 72, 24)
    kw = dict(numDisparities=16, blockSize=5, P2=32000, paths=8)
    with pytest.raises(ref.CostOverflow):
        ref.sgm_compute(L, R, census=(9, 7), **kw)
    flat = np.full((24, 72), 90, np.uint8)
    assert ref.sgm_compute(flat, flat, census=(9, 7), **kw).shape == (24, 72)
    # the invariance pair: census cannot tell the mapped right view from the unmapped one, BT can
    L, R, Rm = cases.lut_pair()
    assert L.max() <= 120 and R.max() <= 120 and np.array_equal(Rm, 2 * R.astype(np.int64) + 10)
    kw = dict(numDisparities=32, blockSize=5, paths=5, speckleWindowSize=0)
    a, b = ref.sgm_compute(L, R, census=(9, 7), **kw), ref.sgm_compute(L, Rm, census=(9, 7), **kw)
    assert np.array_equal(a, b) and (a != -16).mean() > 0.3
    assert (oracle.sgm_compute(L, R, **kw) != oracle.sgm_compute(L, Rm, **kw)).any()
    # preFilterCap 63 against 0 under BT on the switching test's pair: the maps differ, so "applies again" can be seen
    L, R = cases.textured_pair(9400, 110, 28, 7)
    kw = dict(numDisparities=32, blockSize=5, paths=8)
    assert (sgm_cn_ref.sgm_compute_cn(L, R, preFilterCap=63, **kw) != oracle.sgm_compute(L, R, **kw)).any()
