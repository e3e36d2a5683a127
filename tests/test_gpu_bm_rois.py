"""rtdm_bm_compute_device_rois (rules B1-B5): n frames, each under an ROI1 of its own that lies in
device memory, against the existing path -- rtdm_bm_set_roi + rtdm_bm_compute_device per frame on a second handle with the same
parameters.  Both output buffers start as 0x5A5A everywhere and have rows and frames wider than the image; they must be equal
as whole byte arrays, which covers the planes (B1) and everything that must stay untouched (B2: the skipped frame, the bytes
between 2 * width and the pitch, the rows between the frames).  One case also goes against the CPU oracle with the ROI."""
import numpy as np
import pytest

import bm_geom_cases as gc
from stream_gate import StreamGate

pytestmark = pytest.mark.gpu

FILL = 0x5A5A
INT_MIN, INT_MAX = gc.INT_MIN, gc.INT_MAX


@pytest.fixture(scope="module")
def pkg():
    import torch                         # torch first: it brings its own HIP runtime and must initialise before ours
    assert torch.cuda.is_available()
    from conftest import load
    return load()


def seven_rois(W, H, w):
    """whole frame, a small box in two corners, cut by the right and bottom edges, an empty one (skipped), negative x and y,
    narrower than the window (the whole plane FILTERED)"""
    bw, bh = w + 19, w + 12
    return [(0, 0, W, H), (0, 0, bw, bh), (W - 37, H // 2 - 3, 60, H), (10, 10, 0, 20), (-11, -6, W // 2 + 11, H // 2 + 10),
            (W // 3 + 1, 5, w - 2, H - 10), (W - bw, H - bh, bw, bh)]


def cfg(W, H, D, w, minD=0, d12=1, spk=True, roi2=None, norm=False, legacy=0, want=None, pad=8):
    return dict(W=W, H=H, D=D, w=w, minD=minD, d12=d12, spk=spk, roi2=roi2, norm=norm, legacy=legacy, want=want, pad=pad)


def cid(c):
    return "%dx%d_D%d_w%d_min%d_lr%d_spk%d%s%s%s_pad%d" % (c["W"], c["H"], c["D"], c["w"], c["minD"], c["d12"], c["spk"],
                                                          "_roi2" if c["roi2"] else "", "_norm" if c["norm"] else "",
                                                          "_legacy" if c["legacy"] else "", c["pad"])


FAMILIES = [(160, 120, 64, 9, "fast_ring"), (300, 80, 80, 9, "fast_qsad"), (300, 90, 64, 25, "generic_")]
CASES = [cfg(W, H, D, w, d12=d12, spk=spk, want=want) for W, H, D, w, want in FAMILIES for d12 in (1, -1) for spk in (True, False)]
CASES += [cfg(160, 120, 64, 9, minD=4), cfg(160, 120, 64, 9, minD=-3), cfg(160, 120, 64, 9, minD=-3, d12=-1),
          cfg(97, 65, 16, 9, pad=3), cfg(97, 65, 16, 9, minD=4, d12=-1, pad=3), cfg(97, 65, 16, 9, minD=-3, spk=False, pad=3),
          cfg(160, 120, 64, 9, pad=5),                                   # W % 8 == 0 but rows that are not 16-byte aligned
          cfg(120, 82, 16, 7, roi2=(10, 5, 100, 70)), cfg(300, 80, 80, 9, roi2=(-5, -5, 400, 200), d12=-1),
          cfg(160, 120, 64, 9, norm=True), cfg(300, 80, 64, 9, minD=-7, legacy=1),
          cfg(96, 64, 16, 5, minD=-20)]                                  # an ROI left of the frame reaches columns "no ROI" does not


def matcher(pkg, c, max_batch):
    m = pkg.HIPMatcher(numOfDisparities=c["D"], blockSize=c["w"], minDisparity=c["minD"], disp12MaxDiff=c["d12"],
                       speckleWindowSize=100 if c["spk"] else 0, width=c["W"], height=c["H"], max_batch=max_batch,
                       legacy_right_clamp=c["legacy"],
                       preFilterType=pkg.matcher.PREFILTER_NORMALIZED_RESPONSE if c["norm"] else pkg.matcher.PREFILTER_XSOBEL)
    if c["roi2"]:
        m.setROI2(c["roi2"])
    return m


def frames(pkg, c, n):
    import torch
    pairs = [pkg.synth.make_pair(pkg.synth.STREAM_SEED + 31 + 7 * f, c["W"], c["H"], c["D"]) for f in range(n)]
    L = np.stack([p[0] for p in pairs]); R = np.stack([p[1] for p in pairs])
    return L, R, torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()


def out_buffer(c, n, margin=0):
    """[margin + n + margin frames] of (H + 1) rows of W + pad elements, all FILL; the n frames are the middle ones"""
    import torch
    return torch.full((n + 2 * margin, c["H"] + 1, c["W"] + c["pad"]), FILL, dtype=torch.int16, device="cuda")


def per_frame(pkg, m, c, dL, dR, rois, buf, margin=0):
    """the existing path: set_roi + compute_device on every frame alone; a frame with w <= 0 or h <= 0 is left out"""
    W, H = c["W"], c["H"]
    pitch, frame = buf.stride(1) * 2, buf.stride(0) * 2
    for f, r in enumerate(rois):
        if r[2] <= 0 or r[3] <= 0:
            continue
        m.setROI1(r)
        pkg.binding.check(pkg.binding.lib().rtdm_bm_compute_device(
            m._h, 1, dL.data_ptr() + f * W * H, dR.data_ptr() + f * W * H, W, W * H, W, H, buf.data_ptr() + (margin + f) * frame, pitch, frame,
            None), "rtdm_bm_compute_device")


def with_rois(pkg, m, c, dL, dR, d_rois, buf, margin=0, stream=None):
    W, H = c["W"], c["H"]
    pitch, frame = buf.stride(1) * 2, buf.stride(0) * 2
    pkg.binding.check(pkg.binding.lib().rtdm_bm_compute_device_rois(
        m._h, dL.shape[0], dL.data_ptr(), dR.data_ptr(), W, W * H, W, H, d_rois.data_ptr(), buf.data_ptr() + margin * frame, pitch, frame,
        stream), "rtdm_bm_compute_device_rois")


def rois_tensor(rois):
    import torch
    return torch.tensor(rois, dtype=torch.int64).to(torch.int32).cuda().contiguous()


def test_the_roi_set_is_what_the_issue_asks():
    for c in CASES:
        W, H, w = c["W"], c["H"], c["w"]
        rois = seven_rois(W, H, w)
        g = (W, H, c["D"], c["minD"], w, c["d12"], c["roi2"])
        rects = [gc.rect(g, r) for r in rois]
        assert rois[3][2] <= 0 and not rects[5][6]                        # skipped; narrower than the window
        live = [q for i, q in enumerate(rects) if q[6] and i != 3]
        if c["D"] + abs(c["minD"]) < W // 2:
            assert len(live) >= 3, (c, rects)
            assert {q[2] & 1 for q in live} == {0, 1}, (c, rects)         # first valid rows of both parities
        assert any(r[0] % 8 for r in rois) and rois[4][0] < 0 and rois[4][1] < 0
        assert rois[2][0] + rois[2][2] > W and rois[2][1] + rois[2][3] > H


@pytest.mark.parametrize("c", CASES, ids=cid)
def test_every_frame_is_set_roi_and_compute_device_on_it_alone(pkg, c):
    import torch
    n = 7
    rois = seven_rois(c["W"], c["H"], c["w"])
    L, R, dL, dR = frames(pkg, c, n)
    a, b = matcher(pkg, c, n), matcher(pkg, c, 1)
    a.setROI1((3, 3, 40, 40))                                            # the handle's own ROI1 is neither read nor changed (B4)
    got, want = out_buffer(c, n), out_buffer(c, n)
    with_rois(pkg, a, c, dL, dR, rois_tensor(rois), got)
    variant = a.search_variant
    per_frame(pkg, b, c, dL, dR, rois, want)
    torch.cuda.synchronize()
    g, w_ = got.cpu().numpy(), want.cpu().numpy()
    if c["want"]:
        assert variant.startswith(c["want"]), variant
    H, W = c["H"], c["W"]
    filtered = (c["minD"] - 1) * 16
    assert (w_[0, :H, :W] != filtered).any() and (w_[3] == np.int16(FILL)).all() and (w_[5, :H, :W] == filtered).all()
    for f in range(n):
        bad = int((g[f] != w_[f]).sum())
        assert bad == 0, "frame %d (roi %s): %d elements differ, variant %s" % (f, rois[f], bad, variant)
    assert g.tobytes() == w_.tobytes()
    # ... and the handle still computes under the ROI1 its caller set
    one, ref = out_buffer(c, 1), out_buffer(c, 1)
    pkg.binding.check(pkg.binding.lib().rtdm_bm_compute_device(a._h, 1, dL.data_ptr(), dR.data_ptr(), W, W * H, W, H, one.data_ptr(),
                                                               one.stride(1) * 2, one.stride(0) * 2, None), "rtdm_bm_compute_device")
    per_frame(pkg, b, c, dL, dR, [(3, 3, 40, 40)], ref)
    torch.cuda.synchronize()
    assert one.cpu().numpy().tobytes() == ref.cpu().numpy().tobytes()
    a.close(); b.close()


def test_against_the_cpu_oracle_with_an_roi(pkg, oracle):
    import torch
    c = cfg(120, 80, 16, 7, pad=0)
    rois = [(20, 10, 70, 50), (0, 0, 0, 0), (-9, 4, 80, 90)]
    L, R, dL, dR = frames(pkg, c, 3)
    m = matcher(pkg, c, 3)
    out = torch.full((3, 80, 120), FILL, dtype=torch.int16, device="cuda")
    m.compute_device(dL, dR, out, rois=rois_tensor(rois))
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    for f in (0, 2):
        want = oracle.bm_compute(L[f], R[f], numDisparities=16, blockSize=7, roi1=rois[f])
        assert np.array_equal(got[f], want), f
        assert (want != -16).any()
    assert (got[1] == np.int16(FILL)).all()
    m.close()


def test_chunks_of_max_batch(pkg):
    import torch
    c = cfg(160, 120, 64, 9, pad=8)
    n = 5
    rois = seven_rois(160, 120, 9)[:n]
    L, R, dL, dR = frames(pkg, c, n)
    a, b = matcher(pkg, c, 2), matcher(pkg, c, 1)
    got, want = out_buffer(c, n), out_buffer(c, n)
    with_rois(pkg, a, c, dL, dR, rois_tensor(rois), got)
    per_frame(pkg, b, c, dL, dR, rois, want)
    torch.cuda.synchronize()
    assert got.cpu().numpy().tobytes() == want.cpu().numpy().tobytes()
    a.close(); b.close()


HOSTILE = [(INT_MIN, INT_MIN, INT_MAX, INT_MAX), (INT_MAX, INT_MAX, INT_MAX, INT_MAX), (INT_MAX - 100, 3, 200, 20),
           (5, INT_MAX - 7, 60, 100), (INT_MIN, 7, INT_MAX, 40), (20, 10, INT_MAX, INT_MAX), (INT_MIN, INT_MIN, INT_MIN, INT_MIN),
           (-2 ** 30, -2 ** 30, 2 ** 30 + 70, 2 ** 30 + 50), (30, 20, 60, 40), (1, 1, INT_MAX, 1), (-1, -1, 1, INT_MAX)]


@pytest.mark.parametrize("c", [cfg(160, 120, 64, 9, pad=8), cfg(97, 65, 16, 9, d12=-1, pad=3)], ids=cid)
def test_untrusted_rectangles_stay_inside_the_frames(pkg, c):
    """Clamping with valid memory on every side: the frames lie in the middle of a larger allocation of sentinels."""
    import torch
    n, margin = len(HOSTILE), 2
    L, R, dL, dR = frames(pkg, c, n)
    lbig = torch.full((n + 4, c["H"], c["W"]), 0x33, dtype=torch.uint8, device="cuda"); rbig = lbig.clone()
    lbig[2:2 + n] = dL; rbig[2:2 + n] = dR
    a, b = matcher(pkg, c, n), matcher(pkg, c, 1)
    got, want = out_buffer(c, n, margin), out_buffer(c, n, margin)
    d_rois = torch.full((n + 8, 4), 0x7E7E7E7E, dtype=torch.int32, device="cuda")
    d_rois[4:4 + n] = rois_tensor(HOSTILE)
    with_rois(pkg, a, c, lbig[2:2 + n], rbig[2:2 + n], d_rois[4:4 + n], got, margin)
    torch.cuda.synchronize()
    g = got.cpu().numpy()
    assert (g[:margin] == np.int16(FILL)).all() and (g[margin + n:] == np.int16(FILL)).all()
    assert (g[:, c["H"]:, :] == np.int16(FILL)).all() and (g[:, :, c["W"]:] == np.int16(FILL)).all()
    assert (lbig[:2] == 0x33).all() and (lbig[2 + n:] == 0x33).all() and (rbig[:2] == 0x33).all() and (rbig[2 + n:] == 0x33).all()
    assert torch.equal(lbig[2:2 + n], dL) and torch.equal(rbig[2:2 + n], dR)
    assert (d_rois[:4] == 0x7E7E7E7E).all() and (d_rois[4 + n:] == 0x7E7E7E7E).all()
    # Every frame against the host path: with its own rectangle where 32-bit arithmetic does not overflow on it, else with the
    # rectangle cut to +-2^20 on every side, which Python's integers show to have the same geometry (none left: FILTERED).
    geom = (c["W"], c["H"], c["D"], c["minD"], c["w"], c["d12"], c["roi2"])
    filtered = (c["minD"] - 1) * 16
    cut = lambda v: max(-2 ** 20, min(2 ** 20, v))

    def stand_in(r):
        if all(abs(v) <= 2 ** 30 + 100 for v in r):
            return r
        x0, y0, x1, y1 = cut(r[0]), cut(r[1]), cut(r[0] + r[2]), cut(r[1] + r[3])
        q = (x0, y0, x1 - x0, y1 - y0)
        return q if q[2] > 0 and q[3] > 0 and gc.rect(geom, q) == gc.rect(geom, r) else None

    keep = [stand_in(r) if r[2] > 0 and r[3] > 0 else r for r in HOSTILE]
    assert sum(k == r for k, r in zip(keep, HOSTILE)) >= 3 and sum(k is not None and k != r for k, r in zip(keep, HOSTILE)) >= 3
    per_frame(pkg, b, c, dL, dR, [k or (0, 0, 0, 0) for k in keep], want, margin)
    torch.cuda.synchronize()
    w_ = want.cpu().numpy()
    for f, r in enumerate(HOSTILE):
        plane = g[margin + f, :c["H"], :c["W"]]
        if r[2] <= 0 or r[3] <= 0:
            assert (plane == np.int16(FILL)).all(), f
        elif keep[f] is None:
            assert not gc.rect(geom, r)[6] and (plane == filtered).all(), (f, r)
        else:
            assert np.array_equal(g[margin + f], w_[margin + f]), (f, r)
    a.close(); b.close()


# ---- B4: the call enqueues and returns -------------------------------------------------------------------------------------

def test_the_call_does_not_synchronise(pkg):
    import torch
    c = cfg(160, 120, 64, 9, pad=8)
    n = 7
    rois = seven_rois(160, 120, 9)
    L, R, dL, dR = frames(pkg, c, n)
    a, b = matcher(pkg, c, n), matcher(pkg, c, 1)
    d_rois = rois_tensor(rois)
    gate = StreamGate()
    warm = out_buffer(c, n)
    with_rois(pkg, a, c, dL, dR, d_rois, warm, stream=gate.stream.cuda_stream)          # warm-up: modules, attributes
    gate.stream.synchronize()
    got, want = out_buffer(c, n), out_buffer(c, n)
    torch.cuda.synchronize()
    gate.hold()
    with_rois(pkg, a, c, dL, dR, d_rois, got, stream=gate.stream.cuda_stream)           # a call that waited would sit out the 3 s
    gate.event.set()
    gate.stream.synchronize()
    assert gate.released is True
    per_frame(pkg, b, c, dL, dR, rois, want)
    torch.cuda.synchronize()
    assert got.cpu().numpy().tobytes() == want.cpu().numpy().tobytes()
    a.close(); b.close()


def test_python_layer_refuses_with_value_errors(pkg):
    import torch
    c = cfg(160, 120, 64, 9)
    L, R, dL, dR = frames(pkg, c, 2)
    m = matcher(pkg, c, 2)
    out = torch.zeros((2, 120, 160), dtype=torch.int16, device="cuda")
    good = rois_tensor([(0, 0, 160, 120), (5, 5, 60, 60)])
    for bad in (good.to(torch.int64), good[:1], good.reshape(4, 2), torch.cat([good, good], 1)[:, ::2], good.cpu(), [(0, 0, 1, 1)] * 2):
        with pytest.raises(ValueError):
            m.compute_device(dL, dR, out, rois=bad)
    m.compute_device(dL, dR, out, rois=good)
    torch.cuda.synchronize()
    # B5: the refusals of rtdm_bm_compute_device, d_roi1 among the NULL checks, before any device use
    L_ = pkg.binding.lib()
    p, W, H = dL.data_ptr(), 160, 120
    args = lambda **k: [k.get("h", m._h), k.get("n", 2), k.get("l", p), dR.data_ptr(), k.get("pitch", W), W * H, k.get("W", W), H,
                        k.get("roi", good.data_ptr()), k.get("o", out.data_ptr()), k.get("dp", W * 2), k.get("df", W * H * 2), None]
    assert L_.rtdm_bm_compute_device_rois(*args(roi=None)) == -7 and L_.rtdm_bm_compute_device_rois(*args(l=None)) == -7
    assert L_.rtdm_bm_compute_device_rois(*args(o=None)) == -7 and L_.rtdm_bm_compute_device_rois(*args(h=None)) == -7
    assert L_.rtdm_bm_compute_device_rois(*args(n=0, roi=None)) == -7 and L_.rtdm_bm_compute_device_rois(*args(n=0)) == -2
    assert L_.rtdm_bm_compute_device_rois(*args(W=161)) == -2 and L_.rtdm_bm_compute_device_rois(*args(pitch=W - 1)) == -2
    assert L_.rtdm_bm_compute_device_rois(*args(dp=W * 2 - 2)) == -2 and L_.rtdm_bm_compute_device_rois(*args(dp=W * 2 + 1)) == -2
    assert L_.rtdm_bm_compute_device_rois(*args(df=W * H * 2 + 1)) == -2
    m.close()
