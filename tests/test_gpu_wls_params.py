"""The WLS filter's integer half and its handle: drawn radius / threshold / disparity range / ROI parameters with the confidence
bit for bit on maps built to sit on every comparison's edge; parameter changes on a live handle against fresh handles, byte
for byte, and the refused changes; device planes with pitches and frame strides larger than the frame.  No float tolerance
appears here: the ratio F1 / F2 stays with the checks of tests/test_gpu_wls.py."""
import ctypes as C

import numpy as np
import pytest

import wls_ref as ref
from conftest import load
from test_gpu_wls import generic_params, synthetic_maps, wparams
from test_gpu_wls_solver import check_planes

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    import torch                         # torch first: it brings its own HIP runtime and must initialise before ours
    assert torch.cuda.is_available(), "the -m gpu suite needs an MI355X"
    return load()


# ---- e. drawn integer parameters ---------------------------------------------------------------------------------------------------
SHAPES = [(1, 40), (63, 1), (97, 61), (300, 20)]
RADII = (0, 1, 2, 7, 40, 1000)                           # 1000: larger than every frame
THRESHOLDS = (0, 1, 24, 400, 32767)
EMPTY = 11                                               # the set whose ROI is empty on every shape


def drawn_sets(seed=7, count=20):
    rng = np.random.default_rng(seed)
    out = []
    radii = rng.permutation(np.arange(count) % len(RADII))              # every value three times at the least, in drawn places
    thresholds = rng.permutation(np.arange(count) % len(THRESHOLDS))
    for i in range(count):
        out.append(dict(r=RADII[radii[i]], T=THRESHOLDS[thresholds[i]], minD=int(rng.integers(-40, 21)),
                        D=int(rng.integers(16, 257)), off=tuple(int(v) for v in rng.integers(0, 13, 4))))
    return out


SETS = drawn_sets()


def params_at(s, i, W, H):
    """the set's parameters for a W x H frame: the drawn offsets wrap at half the frame's side, so the ROI is empty for the set
    EMPTY only (its left offset is the rest of the width)"""
    l, r, t, b = s["off"]
    l, r, t, b = l % ((W + 1) // 2), r % max(1, W // 2), t % ((H + 1) // 2), b % max(1, H // 2)
    if i == EMPTY:
        l = W - r
    return generic_params(minD=s["minD"], D=s["D"], r=s["r"], off=(l, r, t, b)) | dict(lrc_thresh=s["T"])


def edge_maps(W, H, p, seed):
    """name -> (dL, dR): the maps on which a comparison of W3 / W4 sits on its edge"""
    rng = np.random.default_rng(seed)
    minD, D, T = p["min_disparity"], p["num_disparities"], p["lrc_thresh"]
    invL, invR = (minD - 1) * 16, -(minD + D) * 16
    none = lambda: (np.full((H, W), invL, np.int16), np.full((H, W), invR, np.int16))
    y, x = np.mgrid[0:H, 0:W]
    maps = {}
    dL, dR, _ = synthetic_maps(W, H, minD=minD, D=D, seed=seed)
    maps["synthetic"] = (dL, dR)
    maps["all invalid"] = none()
    # one valid pixel in the middle, |d| < 16 so that x' = x, and its match
    dL, dR = none()
    dL[H // 2, W // 2], dR[H // 2, W // 2] = 5, -5
    maps["one valid"] = (dL, dR)
    # exactly two valid pixels, neighbours, whose range is T and T + 1: disc is 1 and, for a radius of 1 or more, 0
    for extra in (0, 1):
        dL, dR = none()
        lo = 3 if T < 30000 else -16000
        hi = lo + T + extra
        a, b = ((H // 2, W // 2 - 1), (H // 2, W // 2)) if W > 1 else ((H // 2 - 1, 0), (H // 2, 0))
        dL[a], dL[b] = lo, hi
        for (yy, xx), d in ((a, lo), (b, hi)):
            xp = xx - int(d / 16)
            if 0 <= xp < W:
                dR[yy, xp] = -d
        maps["two valid, range T + %d" % extra] = (dL, dR)
    # dL / 16 sends x' to -1, 0, W - 1 and W, row by row, with remainders that truncation drops
    q = np.choose(y % 4, [x + 1, x, x - (W - 1), x - W])
    dL = (16 * q + np.sign(q) * rng.integers(0, 16, (H, W))).astype(np.int16)
    dR = np.full((H, W), invR, np.int16)
    dR[:, 0] = -dL[:, min(W - 1, 2)]
    dR[:, W - 1] = -dL[:, max(0, W - 3)]
    maps["frame edges"] = (dL, dR)
    # negative disparities with a remainder: truncation toward zero gives x' = x + q, floor x + q + 1; one value, so no
    # discontinuity at any T; a match at x + q only
    qn = 1 if W > 1 else 0
    d = -(16 * qn + 7)
    valid = (x + y) % 4 == 0
    dL = np.where(valid, d, invL).astype(np.int16)
    dR = np.full((H, W), invR, np.int16)
    ok = valid & (x + qn < W)
    dR[y[ok], x[ok] + qn] = -d
    maps["negative remainders"] = (dL, dR)
    for dL, dR in maps.values():
        assert dL.dtype == np.int16 and dR.dtype == np.int16
    return maps


def test_the_drawn_sets_cover_the_parameters():
    assert len(SETS) == 20
    assert {s["r"] for s in SETS} == set(RADII) and {s["T"] for s in SETS} == set(THRESHOLDS)
    assert min(s["minD"] for s in SETS) < -20 and max(s["minD"] for s in SETS) > 0
    for W, H in SHAPES:
        assert [i for i, s in enumerate(SETS) if ref.roi(params_at(s, i, W, H), W, H) is None] == [EMPTY]


@pytest.mark.parametrize("i", range(len(SETS)))
def test_drawn_integer_parameters(pkg, i):
    s = SETS[i]
    for W, H in SHAPES:
        p = params_at(s, i, W, H)
        G = synthetic_maps(W, H, seed=3)[2]
        f = pkg.HIPDisparityWLSFilter(wparams(pkg, p), W, H)
        inv = (p["min_disparity"] - 1) * 16
        seen = set()
        for name, (dL, dR) in edge_maps(W, H, p, seed=i + 1).items():
            want = ref.confidence(dL, dR, p)
            seen |= set(np.unique(want))
            if name == "negative remainders" and i != EMPTY:
                # on the reference alone: this map holds both confidence values in every ROI that is not empty
                assert set(np.unique(want)) == {0.0, 255.0}, (name, W, H)
            out, fl = f.filter(dL, G, None, dR, want_float=True)
            conf = f.getConfidenceMap()
            bad = np.argwhere(conf != want)
            assert len(bad) == 0, "%s %dx%d: confidence differs on %d pixels, first at %s" % (name, W, H, len(bad), tuple(bad[0]))
            box = check_planes(out, fl, p)
            if box is None:
                assert (out == inv).all() and (conf == 0).all()
            else:
                # where nothing in the ROI is confident F2 is 0 everywhere and the output is the invalid value
                if not want.any():
                    assert (out == inv).all()
        assert seen == ({0.0} if i == EMPTY else {0.0, 255.0})


# ---- f. live handles ------------------------------------------------------------------------------------------------------------------
LW, LH = 97, 61
P1 = generic_params(minD=0, D=32, r=2, off=(4, 1, 2, 0))
P2 = dict(P1, sigma_color=4.0, lambda_=500.0, num_iter=5, attenuation=0.6, depth_discontinuity_radius=7, lrc_thresh=3,
          roi_left=0, roi_right=6, roi_top=5, roi_bottom=3)


def run(f, maps, use_right=True):
    dL, dR, G = maps
    out, fl = f.filter(dL, G, None, dR if use_right else None, want_float=True)
    return out.tobytes(), fl.tobytes(), f.getConfidenceMap().tobytes()


def fresh(pkg, p, maps, use_right=True):
    return run(pkg.HIPDisparityWLSFilter(wparams(pkg, p), LW, LH), maps, use_right)


def test_parameter_changes_on_a_live_handle(pkg):
    maps = synthetic_maps(LW, LH, seed=21)
    want1, want2 = fresh(pkg, P1, maps), fresh(pkg, P2, maps)
    assert want1 != want2 and want1[2] != want2[2]
    f = pkg.HIPDisparityWLSFilter(wparams(pkg, P1), LW, LH)
    first = run(f, maps)
    f._set(**P2)
    second = run(f, maps)
    f._set(**P1)
    third = run(f, maps)
    assert first == want1 and second == want2 and third == want1
    # every field of P2 alone, so that none is only taken up together with another
    for k in P2:
        if P2[k] != P1[k]:
            q = dict(P1, **{k: P2[k]})
            f._set(**q)
            assert run(f, maps) == fresh(pkg, q, maps), k
    f._set(**P1)
    assert run(f, maps) == want1


def test_confidence_switched_off_and_on_again(pkg):
    maps = synthetic_maps(LW, LH, seed=22)
    off = dict(P1, use_confidence=0)
    f = pkg.HIPDisparityWLSFilter(wparams(pkg, P1), LW, LH)
    first = run(f, maps)
    f._set(**off)
    second = run(f, maps, use_right=False)
    f._set(**P1)
    third = run(f, maps)
    assert first == fresh(pkg, P1, maps) and second == fresh(pkg, off, maps, use_right=False) and third == first
    assert second != first and not np.frombuffer(second[2], np.float32).any()


REFUSED = [dict(sigma_color=0.0), dict(num_iter=0), dict(num_iter=17), dict(attenuation=0.0), dict(attenuation=1.5),
           dict(lambda_=float("nan")), dict(roi_top=-1), dict(min_disparity=1800, num_disparities=256)]


def test_refused_parameters_change_nothing(pkg):
    B = pkg.binding
    lib = B.lib()
    maps = synthetic_maps(LW, LH, seed=23)
    f = pkg.HIPDisparityWLSFilter(wparams(pkg, P2), LW, LH)
    want = run(f, maps)
    fields = lambda w: tuple(getattr(w, k) for k, _ in B.WLSParams._fields_)
    before = B.WLSParams()
    assert lib.rtdm_wls_get_params(f._h, C.byref(before)) == 0
    assert fields(before) == fields(wparams(pkg, P2))
    for change in REFUSED:
        assert lib.rtdm_wls_set_params(f._h, C.byref(wparams(pkg, dict(P2, **change)))) == -1, change     # RTDM_ERR_BAD_PARAM
        now = B.WLSParams()
        assert lib.rtdm_wls_get_params(f._h, C.byref(now)) == 0
        assert fields(now) == fields(before), change
        assert run(f, maps) == want, change
    # the bound of the disparity range itself is accepted
    assert lib.rtdm_wls_set_params(f._h, C.byref(wparams(pkg, dict(P2, min_disparity=1791, num_disparities=256)))) == 0


# ---- g. pitched device planes ------------------------------------------------------------------------------------------------------------
class Plane:
    """n frames of H x W elements inside a larger tensor full of a sentinel: `pad` (rows before, rows after, elements before,
    elements after) around every frame"""

    def __init__(self, torch, dtype, n, H, W, pad, sentinel, data=None):
        t, b, l, r = pad
        self.t, self.l = t, l
        self.big = torch.full((n, H + t + b, W + l + r), sentinel, dtype=dtype, device="cuda")
        self.view = self.big[:, t:t + H, l:l + W]
        if data is not None:
            self.view.copy_(data)
        size = self.big.element_size()
        self.ptr = self.big.data_ptr() + (t * (W + l + r) + l) * size
        self.pitch = (W + l + r) * size
        self.frame = (H + t + b) * (W + l + r) * size
        self.sentinel = sentinel

    def untouched_outside(self, torch):
        keep = torch.ones_like(self.big, dtype=torch.bool)
        keep[:, self.t:self.t + self.view.shape[1], self.l:self.l + self.view.shape[2]] = False
        return bool((self.big[keep] == self.sentinel).all())


@pytest.mark.parametrize("cn", [1, 3])
@pytest.mark.parametrize("optional", [True, False])
def test_pitched_device_planes(pkg, cn, optional):
    import torch
    lib = pkg.binding.lib()
    W, H, mb = 70, 33, 2
    n = 2 * mb + 1
    p = generic_params(off=(4, 1, 2, 0))
    f = pkg.HIPDisparityWLSFilter(wparams(pkg, p), W + 10, H + 7, max_batch=mb)
    maps = [synthetic_maps(W, H, seed=40 + i) for i in range(n)]
    dl = torch.tensor(np.stack([m[0] for m in maps])).cuda()
    dr = torch.tensor(np.stack([m[1] for m in maps])).cuda()
    g = np.stack([m[2] for m in maps])
    if cn == 3:
        g = np.stack([g, np.roll(g, 5, 2), g // 2 + 9], 3)
    dg = torch.tensor(np.ascontiguousarray(g)).cuda()
    # the contiguous call
    out = torch.empty((n, H, W), dtype=torch.int16, device="cuda")
    conf = torch.empty((n, H, W), dtype=torch.float32, device="cuda")
    flt = torch.empty((n, H, W), dtype=torch.float32, device="cuda")
    f.filter_device(dl, dr, dg, out, conf, flt)
    torch.cuda.synchronize()
    assert (conf > 0).any() and (out != -16).any()
    # the same frames as views of larger tensors
    pl = Plane(torch, torch.int16, n, H, W, (1, 2, 3, 4), -31000, dl)
    pr = Plane(torch, torch.int16, n, H, W, (0, 3, 5, 0), -31001, dr)
    pg = Plane(torch, torch.uint8, n, H, W * cn, (2, 1, 7, 6), 0xA5, dg.reshape(n, H, W * cn))
    po = Plane(torch, torch.int16, n, H, W, (3, 1, 1, 8), 0x5A5A)
    pc = Plane(torch, torch.float32, n, H, W, (1, 1, 2, 1), -7.25)
    pf = Plane(torch, torch.float32, n, H, W, (2, 0, 0, 3), 1e30)
    assert pl.pitch > 2 * W and pl.frame > H * pl.pitch and pg.pitch % 2 == 1

    def call(left=pl.pitch, right=pr.pitch, outp=po.pitch, cp=pc.pitch, fp=pf.pitch, lf=pl.frame, cf=pc.frame, opt=optional):
        return lib.rtdm_wls_filter_device(f._h, n, pl.ptr, left, lf, pr.ptr, right, pr.frame, pg.ptr, pg.pitch, pg.frame, cn, W, H,
                                          po.ptr, outp, po.frame, pc.ptr if opt else None, cp, cf, pf.ptr if opt else None, fp,
                                          pf.frame, None)
    assert call() == 0
    torch.cuda.synchronize()
    assert torch.equal(po.view, out)
    for q in (pl, pr, pg, po, pc, pf):
        assert q.untouched_outside(torch)
    if optional:
        assert torch.equal(pc.view.contiguous().view(torch.int32), conf.view(torch.int32))
        assert torch.equal(pf.view.contiguous().view(torch.int32), flt.view(torch.int32))
    else:
        assert bool((pc.big == pc.sentinel).all()) and bool((pf.big == pf.sentinel).all())
    assert torch.equal(pl.view, dl) and torch.equal(pr.view, dr)
    # odd byte pitches and strides of the int16 planes, float pitches and strides that are no multiple of 4: RTDM_ERR_BAD_SIZE
    assert call(left=pl.pitch + 1) == -2 and call(right=pr.pitch + 1) == -2 and call(outp=po.pitch + 1) == -2
    assert call(lf=pl.frame + 1) == -2
    assert call(cp=pc.pitch + 2, opt=True) == -2 and call(fp=pf.pitch + 1, opt=True) == -2 and call(cf=pc.frame + 2, opt=True) == -2
    # ... and pitches below the frame's width
    assert call(left=2 * W - 2) == -2 and call(outp=2 * W - 2) == -2 and call(cp=4 * W - 4, opt=True) == -2
