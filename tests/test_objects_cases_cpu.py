"""The inputs of tests/test_gpu_objects_raw.py without a device: the oracle (oracle/objects_oracle.c) has to be right on
the hostile masks of tests/cc_cases.py and on the HSV frames before a kernel is judged against it, and the cases have to
keep the properties they were made for.  Second opinions: scipy's labelling (bruteforce.external_boxes), Python integers
(bruteforce.rgb2hsv), exact rationals for the two division tables."""
from fractions import Fraction

import numpy as np
import pytest

import bruteforce as bf
import cc_cases as cc

MAX_BOXES = 20000


def n_components(mask, zero_border):
    from scipy import ndimage as ndi
    m = mask != 0
    if zero_border:
        m = m.copy(); m[0, :] = m[-1, :] = False; m[:, 0] = m[:, -1] = False
    return ndi.label(m, structure=np.ones((3, 3), bool))[1]


def cases(*families):
    return [n for n in cc.NAMES if cc.family(n) in families]


def test_the_case_list_is_what_it_says():
    sizes = {m.shape[::-1] for _, m in cc.CASES}
    assert {(64, 64), (257, 131), (131, 257), (300, 70), (70, 300), (384, 384), (8192, 4), (8191, 3), (1, 40), (40, 1)} <= sizes
    assert {(w, 5) for w in (255, 256, 257, 511, 513, 1025)} <= sizes
    for name, m in cc.CASES:
        assert m.dtype == np.uint8 and m.flags.c_contiguous and set(np.unique(m).tolist()) <= {0, 255}, name
        assert 0 < np.count_nonzero(m) < m.size or m.size <= 40, name
    again = dict(cc._build())                                                  # deterministic
    assert all(np.array_equal(again[n], m) for n, m in cc.CASES)
    rgb = cc.paint(cc.BY_NAME["noise45-64x64"])
    assert set(map(tuple, rgb.reshape(-1, 3).tolist())) == {(128, 128, 128), (200, 20, 20)}


@pytest.mark.parametrize("name", cc.NAMES)
def test_oracle_matches_scipy(oracle, name):
    mask = cc.BY_NAME[name]
    for zb in (True, False):
        got = oracle.external_boxes(mask, 1, zb, max_boxes=MAX_BOXES)
        assert len(got) < MAX_BOXES
        assert got == bf.external_boxes(mask, 1, zb), (name, zb)
        assert oracle.external_boxes(mask, 12, zb, max_boxes=MAX_BOXES) == [b for b in got if b[2] * b[3] >= 12]


# Boxes the oracle finds at min_area = 1 with zero_border (True, False); mirroring and transposing change none of them.
N_BOXES = {
    "dots-64x64": (961, 1024), "rings2-64x64": (1, 1), "rings3-64x64": (1, 1), "rings_cut2-64x64": (2, 2),
    "rings_cut3-64x64": (2, 2), "rings_cut_outer2-64x64": (9, 9), "spiral-64x64": (1, 1), "spiral_inv-64x64": (1, 1),
    "comb-64x64": (1, 1), "comb_edge-64x64": (31, 1), "stairs-64x64": (59, 62), "checker-64x64": (1, 1),
    "border-64x64": (533, 542), "border_closed-64x64": (1, 1), "noise45-64x64": (36, 30), "noise60-64x64": (10, 4),
    "dots-257x131": (8320, 8320), "rings2-257x131": (1, 1), "rings3-257x131": (1, 1), "rings_cut2-257x131": (2, 2),
    "rings_cut3-257x131": (2, 2), "rings_cut_outer2-257x131": (17, 17), "spiral-257x131": (1, 1),
    "spiral_inv-257x131": (1, 1), "comb-257x131": (1, 1), "comb_edge-257x131": (128, 1), "stairs-257x131": (128, 130),
    "checker-257x131": (1, 1), "border-257x131": (5147, 5156), "border_closed-257x131": (1, 1),
    "noise45-257x131": (145, 168), "noise60-257x131": (11, 16), "dots-300x70": (5066, 5250), "rings2-300x70": (1, 1),
    "rings3-300x70": (1, 1), "rings_cut2-300x70": (2, 2), "rings_cut3-300x70": (2, 2), "rings_cut_outer2-300x70": (9, 9),
    "spiral-300x70": (1, 1), "spiral_inv-300x70": (1, 1), "comb-300x70": (1, 1), "comb_edge-300x70": (149, 1),
    "stairs-300x70": (69, 71), "checker-300x70": (1, 1), "border-300x70": (3039, 3048), "border_closed-300x70": (1, 1),
    "noise45-300x70": (131, 133), "noise60-300x70": (10, 10), "quilt3-384x384": (9941, 9965),
    "quilt5-384x384": (5329, 5336), "quilt7-384x384": (2747, 2743), "wide-8192x4": (50, 91), "wide-8191x3": (55, 111),
    "wide-255x5": (6, 16), "wide-256x5": (11, 27), "wide-257x5": (22, 16), "wide-511x5": (7, 13), "wide-513x5": (12, 12),
    "wide-1025x5": (14, 30), "wide-1x40": (0, 9), "wide-40x1": (0, 7),
}


def test_box_counts_of_every_case(oracle):
    assert set(N_BOXES) == {n.split("/")[0] for n in cc.NAMES}
    for name, mask in cc.CASES:
        got = tuple(len(oracle.external_boxes(mask, 1, zb, max_boxes=MAX_BOXES)) for zb in (True, False))
        assert got == N_BOXES[name.split("/")[0]], name


# ---- what keeps the cases from going soft ----------------------------------------------------------------------------
@pytest.mark.parametrize("zb", [True, False])
def test_dots_has_far_more_records_than_one_download_holds(oracle, zb):
    W, H = cc.BIG
    want = oracle.external_boxes(cc.BY_NAME["dots-%dx%d" % (W, H)], 1, zb, max_boxes=MAX_BOXES)
    assert len(want) == 8320 > 512
    assert len(want) <= ((W + 1) // 2 + 1) * ((H + 1) // 2 + 1)               # the detector's record capacity
    small = [len(oracle.external_boxes(cc.BY_NAME[n], 1, zb, max_boxes=MAX_BOXES)) for n in cases("dots") if n.endswith("64x64")]
    assert small[0] == (961 if zb else 1024) and min(small) > 512


@pytest.mark.parametrize("name", cases("rings2", "rings3"))
def test_rings_have_one_external_component(oracle, name):
    mask = cc.BY_NAME[name]
    H, W = mask.shape
    n_rings = len(cc.ring_offsets(W, H, int(cc.family(name)[-1])))
    for zb in (True, False):
        assert len(oracle.external_boxes(mask, 1, zb, max_boxes=MAX_BOXES)) == 1
        assert n_components(mask, zb) == n_rings >= 11
    if min(W, H) == 131:
        assert n_rings > 20


@pytest.mark.parametrize("name", cases("rings_cut2", "rings_cut3", "rings_cut_outer2"))
def test_cut_rings_let_the_background_through(oracle, name):
    mask = cc.BY_NAME[name]
    H, W = mask.shape
    fam = cc.family(name)
    closed = cc.rings(W, H, int(fam[-1]))
    n_rings = len(cc.ring_offsets(W, H, int(fam[-1])))
    for zb in (True, False):
        n = len(oracle.external_boxes(mask, 1, zb, max_boxes=MAX_BOXES))
        assert n > len(oracle.external_boxes(closed, 1, zb, max_boxes=MAX_BOXES)) == 1
        assert n == (n_rings // 2 + 1 if "outer" in fam else 2)                # every ring behind a cut, and no other
        assert n_components(mask, zb) == n_rings


@pytest.mark.parametrize("name", cases("spiral", "spiral_inv", "checker", "comb"))
def test_one_component_patterns(oracle, name):
    from scipy import ndimage as ndi
    mask = cc.BY_NAME[name]
    for zb in (True, False):
        assert len(oracle.external_boxes(mask, 1, zb, max_boxes=MAX_BOXES)) == 1 == n_components(mask, zb)
    if cc.family(name) == "spiral":                                            # held together by corners only
        assert ndi.label(mask != 0)[1] > 20


@pytest.mark.parametrize("name", cases("comb_edge"))
def test_zero_border_cuts_the_teeth_loose(oracle, name):
    mask = cc.BY_NAME[name]
    assert len(oracle.external_boxes(mask, 1, False, max_boxes=MAX_BOXES)) == 1
    assert len(oracle.external_boxes(mask, 1, True, max_boxes=MAX_BOXES)) >= 30


@pytest.mark.parametrize("name", cases("stairs"))
def test_stairs_yield_many_boxes(oracle, name):
    for zb in (True, False):
        assert len(oracle.external_boxes(cc.BY_NAME[name], 1, zb, max_boxes=MAX_BOXES)) > 50


@pytest.mark.parametrize("name", cases("border", "border_closed"))
def test_border_cases_depend_on_the_frame(oracle, name):
    mask = cc.BY_NAME[name]
    a, b = (oracle.external_boxes(mask, 1, zb, max_boxes=MAX_BOXES) for zb in (True, False))
    assert a != b
    if cc.family(name) == "border_closed":
        assert b == [(0, 0, mask.shape[1], mask.shape[0])]                     # the closed ring on the frame hides the rest
    else:
        assert len(b) > 10 and any(x == 0 and y > 0 for x, y, _, _ in b)       # first pixels in column 0


@pytest.mark.parametrize("name", cases("quilt3", "quilt5", "quilt7"))
def test_quilt_has_enclosed_components(oracle, name):
    mask = cc.BY_NAME[name]
    for zb in (True, False):
        n_ext = len(oracle.external_boxes(mask, 1, zb, max_boxes=MAX_BOXES))
        assert n_ext > 512 and n_components(mask, zb) - n_ext >= 64


# ---- HSV -------------------------------------------------------------------------------------------------------------
def test_hsv_tables_are_exact_roundings(oracle):
    sdiv, hdiv = oracle.hsv_tables()
    assert sdiv[0] == 0 and hdiv[0] == 0
    for i in range(1, 256):
        for tab, q in ((sdiv, Fraction(255 << 12, i)), (hdiv, Fraction(180 << 12, 6 * i))):
            assert q - int(q) != Fraction(1, 2), i                             # no tie: every rounding rule agrees
            assert int(tab[i]) == int(q + Fraction(1, 2)), i
        # the integer forms of k_hsv_tabs
        assert ((255 << 12) * 2 + i) // (2 * i) == sdiv[i] and ((180 << 12) * 2 + 6 * i) // (12 * i) == hdiv[i]


@pytest.fixture(scope="module")
def hsv(oracle):
    rgb = cc.hsv_frame()
    return rgb, oracle.rgb2hsv(rgb)


def test_hsv_frame_holds_what_it_says():
    hue, sat, rgb = cc.hue_block(), cc.sat_block(), cc.hsv_frame()
    assert len(hue) == 6 * 65536 and len(sat) == 3 * 32896 == cc.SAT_W * cc.SAT_H
    assert rgb.shape == (481, 1024, 3) and np.array_equal(rgb.reshape(-1, 3)[:len(hue)], hue)
    assert np.array_equal(rgb.reshape(-1, 3)[len(hue):len(hue) + len(sat)], sat)
    assert np.array_equal(cc.sat_frame().reshape(-1, 3), sat)
    h = hue.astype(int)
    for s in range(3):                                                         # sector s: channel s is a maximum
        blk = h[s * 131072:(s + 1) * 131072]
        assert (blk[:, s] == blk.max(1)).all()
        d = blk.max(1) - blk.min(1)
        off = blk[:, (s + 1) % 3] - blk[:, (s + 2) % 3]
        pairs = set(zip(d[:65536].tolist(), off[:65536].tolist()))
        assert pairs == {(dd, o) for dd in range(256) for o in range(-dd, dd + 1)}
        assert (blk[:65536].min(1) == 0).all() and (blk[65536:].max(1) == 255).all()
    assert (h[:, 0] == h[:, 1]).any() and (h[:, 1] == h[:, 2]).any() and (h[:, 0] == h[:, 2]).any()      # the ties are in
    s3 = sat.astype(int).reshape(3, 32896, 3)
    for s in range(3):
        assert (s3[s][:, s] == s3[s].max(1)).all()
        assert len(set(zip(s3[s].max(1).tolist(), s3[s].min(1).tolist()))) == 32896


def test_hsv_oracle_matches_python_ints_on_a_sample(hsv):
    rgb, planes = hsv
    idx = np.random.default_rng(21).choice(rgb.shape[0] * rgb.shape[1], 20000, replace=False)
    px = rgb.reshape(-1, 3)[idx].reshape(100, 200, 3)
    assert np.array_equal(planes.reshape(-1, 3)[idx].reshape(100, 200, 3), bf.rgb2hsv(px))


def test_hsv_frame_covers_every_value(oracle, hsv):
    _, planes = hsv
    assert set(np.unique(planes[..., 0]).tolist()) == set(range(180))          # every hue, none of 180 and above
    assert set(np.unique(planes[..., 1]).tolist()) == set(range(256))
    assert set(np.unique(planes[..., 2]).tolist()) == set(range(256))
    sat = oracle.rgb2hsv(cc.sat_frame())
    assert set(np.unique(sat[..., 1]).tolist()) == set(range(256)) and set(np.unique(sat[..., 2]).tolist()) == set(range(256))


def test_random_ranges_are_what_they_say(oracle):
    rr = cc.random_ranges()
    assert len(rr) == 32 and rr[0] == (oracle.HSV_LOW, oracle.HSV_HIGH)
    assert any(lo[c] > hi[c] for lo, hi in rr[1:2] for c in range(3))
    rgb = cc.sat_frame()
    hits = [np.count_nonzero(oracle.hsv_inrange(rgb, lo, hi)) for lo, hi in rr]
    assert hits[1] == 0 and sum(0 < h < cc.SAT_W * cc.SAT_H for h in hits) >= 16
