"""StereoSGBM's MODE_SGBM_3WAY (rtdm_sgm_set_mode, rules T1-T8 of DESIGN.md section 4.21) on the CPU side: the NumPy reference
sgm_3way_ref.py anchored to sgm_hh4_ref's recurrence (itself anchored to the C oracle's), the stripe table of the product's own
host function (rtdm_sgm_stripes.h, through the stand-alone program tests/sgm_stripes_host.cpp) against T1 restated here, the
setter's refusals that need no device, the Python and C++ layers, and -- so that no GPU case of test_gpu_sgm_3way.py can pass
vacuously -- what those cases rest on: the reference finds disparities on every textured pair, four stripes give another map
than one, T3's floor shows in the map, the saturated pair saturates and the refused pair is refused.  Parity with
cv::StereoSGBM itself is unpinned."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import sgm_3way_cases as cases
import sgm_3way_ref as ref
import sgm_hh4_ref
from conftest import PKG, ROOT, load
from test_wls_adapter import MATCHER, SHIM

HOST = os.path.join(ROOT, PKG, "host")
CSRC = os.path.join(ROOT, PKG, "csrc")

# W, H, D, blockSize: the anchors' pairs
ANCHORS = [(96, 40, 16, 5), (128, 64, 32, 5), (160, 65, 32, 9), (80, 9, 16, 3)]


def _volumes(W, H, D, bs):
    L, R = cases.pair(100 + W + H, W, H, 6)
    p = ref.params_of(numDisparities=D, blockSize=bs)
    pix = ref.pixel_costs(L, R, p)
    Cc, _ = ref.block_costs(pix, bs)
    return pix, Cc


@pytest.mark.parametrize("W,H,D,bs", ANCHORS)
def test_one_stripe_is_the_three_direction_aggregate(oracle, W, H, D, bs):
    """with one stripe T1-T5 are R4 + R5 over (1, 0), (-1, 0), (0, 1): sgm_hh4_ref.aggregate, byte for byte"""
    pix, Cc = _volumes(W, H, D, bs)
    S1, _ = ref.aggregate(pix, Cc, 600, 2400, bs, nstripes=1)
    assert np.array_equal(S1, sgm_hh4_ref.aggregate(Cc, 600, 2400, ((1, 0), (-1, 0), (0, 1))))


@pytest.mark.parametrize("W,H,D,bs", ANCHORS)
def test_stripe_0_is_the_one_stripe_result_and_the_others_are_not(oracle, W, H, D, bs):
    pix, Cc = _volumes(W, H, D, bs)
    S1, _ = ref.aggregate(pix, Cc, 600, 2400, bs, nstripes=1)
    S4, _ = ref.aggregate(pix, Cc, 600, 2400, bs)
    st = ref.stripes(H, bs)
    assert np.array_equal(S4[st[0][1]:st[0][2]], S1[st[0][1]:st[0][2]])
    for a, o, e in st[1:]:
        if a == 0:                                              # the chain starts where the frame's does: the same costs
            assert np.array_equal(S4[o:e], S1[o:e])
        else:
            assert all((S4[y] != S1[y]).any() for y in range(o, e)), (a, o, e)
    assert any(a > 0 and o < e for a, o, e in st[1:])


def test_the_floor_changes_the_costs_of_every_later_stripe(oracle):
    W, H, D, bs = ANCHORS[0]
    pix, Cc = _volumes(W, H, D, bs)
    S4, cmax = ref.aggregate(pix, Cc, 600, 2400, bs)
    Sn, cmaxn = ref.aggregate(pix, Cc, 600, 2400, bs, floor=False)
    st = ref.stripes(H, bs)
    assert np.array_equal(S4[:st[0][2]], Sn[:st[0][2]])
    for a, o, e in st[1:]:
        assert a > 0 and all((S4[y] != Sn[y]).any() for y in range(o, e))
    assert cmaxn == int(Cc.max()) and cmax >= cmaxn
    # C' by T3's words, for one stripe: the window's rows above a count as row a
    a, o, e = st[2]
    h = ref.row_sums(pix, bs)
    Cw = ref.warm_costs(h, a, e, bs)
    R = bs // 2
    assert len(Cw) == R and o - a >= R + 1
    for i in range(R):
        want = sum(h[max(a + i + j, a)] for j in range(-R, R + 1))
        assert np.array_equal(Cw[i], want)
    assert np.array_equal(sum(h[a + R + j] for j in range(-R, R + 1)), Cc[a + R].astype(np.int64))      # from row a + R on C' = C


def test_the_ceil_identity():
    """(sz + 9) // 10 is the library's (int)ceil(0.1 * sz) in IEEE double for every sz <= 200000"""
    sz = np.arange(0, 200001)
    assert np.array_equal(np.ceil(0.1 * sz.astype(np.float64)).astype(np.int64), (sz + 9) // 10)
    assert all(int(math.ceil(0.1 * s)) == (s + 9) // 10 for s in (1, 9, 10, 11, 180, 199999, 200000))


def test_stripe_examples():
    assert [s[0] for s in ref.stripes(720, 5)] == [0, 159, 339, 519]
    assert ref.stripes(5, 5) == [(0, 0, 2), (0, 2, 4), (0, 4, 5), (2, 5, 5)]


@pytest.fixture(scope="module")
def stripes_exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("sgm_stripes") / "sgm_stripes_host")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-Werror", "-I", CSRC,
                           os.path.join(ROOT, "tests", "sgm_stripes_host.cpp"), "-o", out])
    return out


def test_the_products_stripe_table(stripes_exe):
    """the host function the launch calls, against T1 restated in sgm_3way_ref.stripes"""
    combos = [(H, bs) for H in list(range(1, 10)) + [64, 65, 404, 720] for bs in (1, 5, 13)]
    p = subprocess.run([stripes_exe] + [str(v) for c in combos for v in c], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    lines = p.stdout.splitlines()
    assert len(lines) == len(combos)
    for (H, bs), line in zip(combos, lines):
        v = [int(t) for t in line.split()]
        assert v[:2] == [H, bs] and v[2] == min(bs // 2, H)
        got = [tuple(v[3 + 3 * s:6 + 3 * s]) for s in range(4)]
        assert got == ref.stripes(H, bs), (H, bs)
        # what the kernels rely on: a <= o <= e <= H, stripes tile [0, H), and a stripe with a > 0 warms up for more than R rows
        assert all(0 <= a <= o <= e <= H for a, o, e in got)
        assert got[0][1] == 0 and got[3][2] == H and all(got[s][2] == got[s + 1][1] for s in range(3))
        assert all(o - a >= bs // 2 + 1 for a, o, e in got if a > 0 and o < e)
    assert subprocess.run([stripes_exe, "1"], capture_output=True).returncode == 2


def test_header_and_exports_carry_the_setter():
    B = load("binding")
    text = open(os.path.join(ROOT, "include", "rtdm.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+rtdm_sgm_set_mode\s*\(\s*rtdm_sgm\s*\*\s*sg\s*,\s*int\s+mode\s*\)\s*;", code)
    assert re.search(r"\bint\s+rtdm_sgm_get_mode\s*\(\s*const\s+rtdm_sgm\s*\*\s*sg\s*,\s*int\s*\*\s*mode\s*\)\s*;", code)
    for name, v in (("SGBM", 0), ("HH", 1), ("SGBM_3WAY", 2), ("HH4", 3)):
        assert re.search(r"#define\s+RTDM_SGM_MODE_%s\s+%d\b" % (name, v), code), name
    assert "rtdm_sgm_set_mode" in B.EXPORTS and "rtdm_sgm_get_mode" in B.EXPORTS
    L = C.CDLL(B.LIB_PATH)
    assert hasattr(L, "rtdm_sgm_set_mode") and hasattr(L, "rtdm_sgm_get_mode")
    assert C.sizeof(B.SGMParams) == 40 and B.lib().rtdm_abi_version() == 3
    for name in ("T1", "T2", "T3", "T4", "T5", "T6", "T7", "T8"):
        assert re.search(r"\b%s\b" % name, text), name
    assert "unpinned" in text


def test_rules_are_written_down_with_parity_unpinned():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = design[design.index("4.21"):]
    for name in ("T1", "T2", "T3", "T4", "T5", "T6", "T7", "T8"):
        assert re.search(r"\b%s\b" % name, sec), name
    assert "unpinned" in sec and "vert3" in design
    assert "rtdm_sgm_set_mode" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "MODE_SGBM_3WAY" in open(os.path.join(ROOT, "README.md")).read()


def test_null_handle_is_refused():
    L = load("binding").lib()
    m = C.c_int(9)
    for mode in (0, 1, 2, 3, 4, -1):
        assert L.rtdm_sgm_set_mode(None, mode) == -7                                # NULL is found first
    assert L.rtdm_sgm_get_mode(None, C.byref(m)) == -7 and m.value == 9
    assert L.rtdm_sgm_get_mode(None, None) == -7


def test_python_set_mode_is_checked_before_the_library():
    import torch
    pkg = load()
    M = pkg.HIPSemiGlobalMatcher
    assert (M.MODE_SGBM, M.MODE_HH, M.MODE_SGBM_3WAY, M.MODE_HH4) == (0, 1, 2, 3)
    assert callable(M.setMode) and callable(M.getMode)
    kw = dict(numOfDisparities=16, width=64, height=16)
    if torch.cuda.is_available():
        m = M(paths=5, **kw)
        try:
            for bad in (4, -1, None, "3way", True, 2.5, 2.0, [2], {}):
                with pytest.raises(ValueError):
                    m.setMode(bad)
            assert m.mode == M.MODE_SGBM and m.getMode() == M.MODE_SGBM
            m.setMode(M.MODE_SGBM_3WAY)
            assert m.mode == M.MODE_SGBM_3WAY and m.params.paths == 3 and m.getMode() == M.MODE_SGBM_3WAY
        finally:
            m.close()
    else:
        with pytest.raises(pkg.binding.RtdmError) as e:
            M(paths=5, **kw)
        assert e.value.status == -3
    # the creation door stays shut, with or without a device
    for shut in (dict(mode=M.MODE_SGBM_3WAY), dict(paths=3)):
        with pytest.raises(pkg.binding.RtdmError) as e:
            M(**dict(kw, **shut))
        assert e.value.status == -6


def test_adapter_with_set_mode_compiles(tmp_path):
    """sgbm-hip.h with setMode, in the reference's dialect"""
    (tmp_path / "opencv2").mkdir()
    (tmp_path / "opencv2" / "opencv.hpp").write_text(SHIM)
    sm = tmp_path / "stereo-matcher"
    sm.mkdir()
    (sm / "stereo-matcher.h").write_text(MATCHER)
    (sm / "sgbm-hip.h").write_text(open(os.path.join(HOST, "sgbm-hip.h")).read())
    user = tmp_path / "user.cpp"
    user.write_text(r"""
#include "stereo-matcher/sgbm-hip.h"
int threeway(HIPSemiGlobalMatcher& m) { return m.setMode(rtdm::MODE_SGBM_3WAY); }
int back(HIPSemiGlobalMatcher& m) { return m.setMode(rtdm::MODE_SGBM); }
int read(const HIPSemiGlobalMatcher& m) { return m.getMode(); }
int core(HIPSemiGlobalMatcher& m) { return m.getCore()->setMode(RTDM_SGM_MODE_HH4) + m.getCore()->mode(); }
static_assert(RTDM_SGM_MODE_SGBM == rtdm::MODE_SGBM && RTDM_SGM_MODE_HH == rtdm::MODE_HH &&
              RTDM_SGM_MODE_SGBM_3WAY == rtdm::MODE_SGBM_3WAY && RTDM_SGM_MODE_HH4 == rtdm::MODE_HH4, "cv::StereoSGBM's values");
""")
    for src in (str(user), os.path.join(HOST, "sgbm-hip.cpp")):
        r = subprocess.run(["g++", "-std=c++11", "-Wall", "-Werror", "-fsyntax-only", "-I", str(tmp_path), "-I", HOST,
                            "-I", os.path.join(ROOT, "include"), src], capture_output=True, text=True)
        assert r.returncode == 0, src + "\n" + r.stderr


# ---- the GPU tests' inputs, checked where no GPU is needed ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def maps(oracle):
    """name -> (four-stripe map, one-stripe map, map without T3's floor) of every textured case, computed once"""
    out = {}
    for c in cases.CASES:
        L, R = c.frames()
        out[c.name] = (c.want(L, R), c.want(L, R, nstripes=1), c.want(L, R, floor=False))
    return out


@pytest.mark.parametrize("name", [c.name for c in cases.CASES])
def test_textured_cases_find_disparities(maps, name):
    c = cases.BY_NAME[name]
    want = maps[name][0]
    assert want.shape == (c.H, c.W) and (c.W + min(c.minD, 0)) - max(c.minD + c.D, 0) > 0
    assert ref.valid_share(want, c.minD, c.D) >= 0.30
    dom = want[:, max(c.minD + c.D, 0):c.W + min(c.minD, 0)]
    assert (np.abs(dom[dom != (c.minD - 1) * 16] - 16 * (c.minD + c.shift)) <= 8).mean() > 0.5


@pytest.mark.parametrize("name", cases.STRIPE_CASES)
def test_four_stripes_give_another_map_than_one(maps, name):
    assert (maps[name][0] != maps[name][1]).any()


@pytest.mark.parametrize("name", cases.FLOOR_CASES)
def test_the_floor_shows_in_the_map(maps, name):
    assert (maps[name][0] != maps[name][2]).any()


def test_the_asserted_case_sets_leave_out_only_what_cannot_show():
    """every case with a stripe that warms up is in STRIPE_CASES, every such case with a C' in FLOOR_CASES -- every blockSize-5
    case but the two frames too low to have such a stripe, both larger windows, and every pixel-cost form (gray, 16-bit, colour,
    census) -- and the cases left out give the same map either way"""
    names = {c.name for c in cases.CASES}
    assert names - set(cases.STRIPE_CASES) == {"h5", "h3_empty_stripe"}
    assert names - set(cases.FLOOR_CASES) == {"h5", "h3_empty_stripe", "bs1_no_warm"}
    for n in ("colour", "cap63", "census97", "bs9_unfused", "bs19_checked", "d256", "h9"):
        assert n in cases.FLOOR_CASES
    for n in ("h5", "h3_empty_stripe"):
        c = cases.BY_NAME[n]
        assert all(a == 0 for a, o, e in ref.stripes(c.H, c.bs) if o < e)


def test_small_frames_cover_what_they_are_for():
    assert ref.stripes(9, 5) == [(0, 0, 3), (0, 3, 6), (2, 6, 9), (5, 9, 9)]         # overlap 4 > stripe 3; an empty last stripe
    assert ref.stripes(3, 5)[3] == (0, 3, 3) and all(a == 0 for a, _, _ in ref.stripes(3, 5))
    assert [s[0] for s in ref.stripes(65, 19)] == [0, 5, 22, 39]
    b = cases.BY_NAME["bs19_checked"]
    assert 93 * b.bs * b.bs + b.P2 > 32767                                            # T8 is live there


def test_saturated_and_refused_inputs(oracle):
    L, R = cases.saturated_pair()
    kw = cases.saturated_params()
    p = ref.params_of(**kw)
    pix = ref.pixel_costs(L, R, p)
    Cc, _ = ref.block_costs(pix, p.blockSize)
    S, cmax = ref.aggregate(pix, Cc, kw["P1"], kw["P2"], p.blockSize)
    assert cmax + kw["P2"] <= 32767
    sat = S.min(axis=2) >= 32767
    assert sat.sum() > 100                                                             # the input does what it is built for
    want = ref.sgm_compute(L, R, **kw)
    dom = want[:, 16:]
    assert (dom == -16).sum() > 100 and (dom != -16).mean() > 0.9                     # uniqueness 0: no winner is the one way to be invalid
    r = cases.REFUSED
    with pytest.raises(ref.CostOverflow):
        ref.sgm_compute(*cases.noise_pair(5, r["W"], r["H"]), numDisparities=r["D"], blockSize=r["bs"], P2=r["P2"])


def test_the_pair_refused_through_a_warm_up_cost_alone(oracle):
    """T8 on a C': no frame-relative block cost of the pair passes the limit, one C' does -- by the arithmetic in sgm_3way_cases.py"""
    r = cases.WARM_REFUSED
    L, R = cases.warm_refused_pair()
    kw = cases.warm_refused_params()
    limit = 32767 - r["P2"]
    assert 93 * r["bs"] * r["bs"] + r["P2"] > 32767                                   # the check is live
    assert ref.stripes(r["H"], r["bs"])[2][0] == r["band"][0]                         # the band starts at stripe 2's first source row
    p = ref.params_of(**kw)
    pix = ref.pixel_costs(L, R, p)
    Cc, cmax = ref.block_costs(pix, r["bs"])
    _, cmax_warm = ref.aggregate(pix, Cc, 600, r["P2"], r["bs"])
    assert cmax == 9 * 19 * 63 <= limit < 18 * 19 * 63 == cmax_warm
    with pytest.raises(ref.CostOverflow):
        ref.sgm_compute(L, R, **kw)
    assert ref.sgm_compute(L, R, floor=False, **kw).shape == L.shape                  # without T3's floor nothing refuses it
