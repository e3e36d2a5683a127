"""k_wls_solve on the device, alone: one pass in one direction per line length, line count, ROI placement, lambda and weight
structure against float64 Thomas by the derived bound (tests/wls_solve_model.py); passes whose weights
are all zero bit for bit; drawn solver parameters on 2-D frames by the summed bound; and the int16 plane as the rounded float
plane everywhere.  Every filter here runs without the confidence, so the float plane is the solver's own fp32 result."""
import numpy as np
import pytest

import wls_ref as ref
import wls_solve_model as M
from conftest import load
from test_gpu_wls import synthetic_maps, wparams

pytestmark = pytest.mark.gpu

WORST = {}                                               # (direction, NCH) -> the device's largest c so far


@pytest.fixture(scope="module")
def pkg():
    import torch                         # torch first: it brings its own HIP runtime and must initialise before ours
    assert torch.cuda.is_available(), "the -m gpu suite needs an MI355X"
    return load()


def params(lambda_=8000.0, sigma_color=1.5, num_iter=1, attenuation=0.25, off=(0, 0, 0, 0)):
    return dict(lambda_=lambda_, sigma_color=sigma_color, lrc_thresh=24, depth_discontinuity_radius=2, min_disparity=M.MIN_D,
                num_disparities=M.NUM_D, roi_left=off[0], roi_right=off[1], roi_top=off[2], roi_bottom=off[3], num_iter=num_iter,
                attenuation=attenuation, use_confidence=0)


def check_planes(out, fl, p):
    """(d): the int16 plane is the float plane rounded half to even and saturated; outside the ROI both hold the invalid value"""
    H, W = out.shape
    inv = (p["min_disparity"] - 1) * 16
    assert np.array_equal(out, np.clip(np.rint(fl), -32768, 32767).astype(np.int16))
    inside = np.zeros((H, W), bool)
    box = ref.roi(p, W, H)
    if box:
        inside[box[2]:box[3], box[0]:box[1]] = True
    assert (out[~inside] == inv).all() and (fl[~inside] == np.float32(inv)).all()
    return box


# ---- a. one pass, one direction ---------------------------------------------------------------------------------------------------
_handles = {}


def handle(pkg, direction):
    """one handle per direction, larger than every frame it serves: the planes' pitch differs from the frame's width"""
    if direction not in _handles:
        size = (4096, 24) if direction == "rows" else (24, 4096)
        _handles[direction] = pkg.HIPDisparityWLSFilter(wparams(pkg, params()), *size)
    return _handles[direction]


def embed(rng, roi, top, bottom, left, right, hi):
    """the ROI's plane inside a frame of random values"""
    h, w = roi.shape[:2]
    full = rng.integers(0, hi, (h + top + bottom, w + left + right) + roi.shape[2:]).astype(roi.dtype)
    full[top:top + h, left:left + w] = roi
    return full


def on_device(f, dL, G):
    """filter_device on one frame: the host call copies a frame row by row, which for 4096 rows of a few pixels takes longest"""
    import torch
    out = torch.empty((1,) + dL.shape, dtype=torch.int16, device="cuda")
    fl = torch.empty((1,) + dL.shape, dtype=torch.float32, device="cuda")
    f.filter_device(torch.from_numpy(dL[None]).cuda(), None, torch.from_numpy(G[None]).cuda(), out, None, fl)
    torch.cuda.synchronize()
    return out[0].cpu().numpy(), fl[0].cpu().numpy()


@pytest.mark.parametrize("n", M.GPU_LENGTHS)
@pytest.mark.parametrize("direction", ["rows", "columns"])
def test_one_pass_against_float64_thomas(pkg, direction, n):
    """Rows: every vertical pair of the guide differs by 150 or more in each channel, wv == 0, the column pass is the exact
    identity and each ROI row is one 1-D solve.  Columns: the same frames transposed."""
    rng = np.random.default_rng(100 + n)
    f = handle(pkg, direction)
    runs, wts, lams, rhs, got = [], [], [], [], []
    for count in (1, 3, 17):
        for placed in (False, True):
            # along the line 2 before and 3 after where the handle has room, across it 1 before and 2 after
            al, ar = ((2, 3) if n + 5 <= 4096 else (0, 0)) if placed else (0, 0)
            ct, cb = (1, 2) if placed else (0, 0)
            for name, (cn, sigma, _, _) in M.STRUCTURES.items():
                if name == "sigma10" and count > 1:
                    continue
                g = M.row_guide(rng, name, count, n)
                d = M.disparities(rng, count, n, first_step=placed)
                wh, wv = M.guide_weights(g, sigma)
                assert not wv.any()
                G, dL = embed(rng, g, ct, cb, al, ar, 256), embed(rng, d, ct, cb, al, ar, 4000)
                off = (al, ar, ct, cb)
                if direction == "columns":
                    G, dL = G.swapaxes(0, 1).copy(order="C"), dL.T.copy(order="C")        # fresh strides, also for one line
                    off = (ct, cb, al, ar)
                for lam in M.LAMBDAS:
                    p = params(lambda_=2.0 * lam, sigma_color=sigma, off=off)
                    f._set(**p)
                    out, fl = f.filter(dL, G, None, None, want_float=True) if direction == "rows" else on_device(f, dL, G)
                    x0, x1, y0, y1 = check_planes(out, fl, p)
                    u = fl[y0:y1, x0:x1]
                    u = u.T if direction == "columns" else u
                    assert u.shape == (count, n)
                    lp, = M.pass_lambdas(p)
                    assert lp == np.float32(lam)
                    wts.append(wh); lams.append(np.full(count, lp)); rhs.append(d.astype(np.float32)); got.append(u)
                    runs += [(count, placed, name, lam)] * count
    wt, lam, fr, u = np.concatenate(wts), np.concatenate(lams), np.concatenate(rhs)[..., None], np.concatenate(got)[..., None]
    c = M.c_of(u, M.ref64(wt, lam, fr), wt, lam, fr)
    i = int(c.argmax())
    nch = M.wls_nch(n)
    print("k_wls_solve<%d> %s length %d: largest c %.3f at (lines, placed, weights, lambda) = %s" % (nch, direction, n, c[i], runs[i]))
    WORST[direction, nch] = max(WORST.get((direction, nch), 0.0), float(c[i]))
    assert c[i] <= M.C_DEV_MAX, "line %d of %s misses the bound: c = %.4g" % (i, runs[i], c[i])
    # a pass with lambda 0 and a line of one element return the input bit for bit
    exact = (lam == 0) | (n == 1)
    assert np.array_equal(u[exact].view(np.int32), fr[exact].view(np.int32))


def test_the_lengths_reach_every_solver_shape():
    assert {M.wls_nch(n) for n in M.GPU_LENGTHS} == {4, 8, 16, 32, 64}


@pytest.fixture(scope="module", autouse=True)
def report():
    """after the module's tests: the device's largest c per instantiation and direction, for the run log"""
    yield
    for (direction, nch), c in sorted(WORST.items()):
        print("\nk_wls_solve<%d> %s: largest c %.3f (held to %g)" % (nch, direction, c, M.C_DEV_MAX), end="")


# ---- b. zero weights ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", [(257, 33), (65, 130)])
def test_zero_weights_return_the_input_bit_for_bit(pkg, W, H):
    rng = np.random.default_rng(W)
    G = M.zero_weight_guide(rng, H, W)
    dL = rng.integers(-64, 4001, (H, W)).astype(np.int16)
    f = pkg.HIPDisparityWLSFilter(wparams(pkg, params()), W + 3, H + 2)
    for off in ((0, 0, 0, 0), (3, 1, 2, 4)):
        for num_iter in (1, 3, 16):
            for lam in (0.3, 8000.0, 1e5):
                p = params(lambda_=lam, num_iter=num_iter, attenuation=0.9, off=off)
                f._set(**p)
                out, fl = f.filter(dL, G, None, None, want_float=True)
                x0, x1, y0, y1 = check_planes(out, fl, p)
                assert np.array_equal(fl[y0:y1, x0:x1].view(np.int32), dL[y0:y1, x0:x1].astype(np.float32).view(np.int32))


# ---- c. drawn solver parameters on 2-D frames -------------------------------------------------------------------------------------
SETS = M.drawn_sets()
KEPT = [i for i, p in enumerate(SETS) if M.says_something(p)]


def test_the_drawn_sets_cover_the_solver():
    kept = [SETS[i] for i in KEPT]
    assert len(SETS) == 24 and len(kept) >= 16
    assert any(p["num_iter"] >= 8 for p in kept) and any(p["num_iter"] == 1 for p in kept)


@pytest.fixture(scope="module")
def frames2d():
    out = {}
    for W, H in ((150, 40), (257, 17), (70, 129)):
        dL, _, G = synthetic_maps(W, H, minD=M.MIN_D, D=M.NUM_D, seed=W)
        rng = np.random.default_rng(H)
        G3 = np.stack([G, np.roll(G, 3, 1), (G.astype(np.int32) * 3 // 4 + rng.integers(0, 9, (H, W))).astype(np.uint8)], 2)
        out[W, H] = (dL, G, np.ascontiguousarray(G3))
    return out


@pytest.mark.parametrize("i", KEPT)
def test_drawn_solver_parameters(pkg, frames2d, i):
    p = SETS[i]
    table = ref.lut(p["sigma_color"]).astype(np.float64)
    for (W, H), (dL, G1, G3) in frames2d.items():
        f = pkg.HIPDisparityWLSFilter(wparams(pkg, p), W + 7, H + 1)
        for G in (G1, G3):
            out, fl = f.filter(dL, G, None, None, want_float=True)
            x0, x1, y0, y1 = box = check_planes(out, fl, p)
            d = dL[y0:y1, x0:x1].astype(np.float64)
            wh, wv = ref.weights(G, table, box)
            want = M.fgs(d[..., None], wh, wv, p)[..., 0]
            fmax = np.abs(d).max()
            tol = M.C_DEV_MAX * M.EPS * fmax * sum((1 + 4 * float(l) * wh.max()) + (1 + 4 * float(l) * wv.max()) for l in M.pass_lambdas(p))
            assert tol <= 2.0 ** -8 * fmax
            u = fl[y0:y1, x0:x1].astype(np.float64)
            err = np.abs(u - want).max()
            print("set %d (lambda %.4g, sigma %.3g, %d iterations, attenuation %.3g) %dx%d cn %d: c = %.3f" % (
                i, p["lambda_"], p["sigma_color"], p["num_iter"], p["attenuation"], W, H, G.ndim == 3 and 3 or 1,
                M.C_DEV_MAX * err / tol))
            assert err <= tol
            assert d.min() - tol <= u.min() and u.max() <= d.max() + tol
