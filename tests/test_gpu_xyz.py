"""reprojectImageTo3D and the point cloud on the device (rtdm_xyz_*, rtdm_bm_compute_cloud) against tests/xyz_ref.py.

The tolerance is zero, by derivation: every operation of X1-X3 is an IEEE-correctly rounded double
operation on both sides, in the same order, followed by one rounding to float.  Dense maps are compared with
np.array_equal(equal_nan=True), clouds by their raw bytes, and every byte outside what a call may write must keep its
sentinel."""
import ctypes as C

import numpy as np
import pytest

import xyz_ref as ref
from conftest import load

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (63, 1), (65, 2), (257, 5), (2049, 3), (4096, 2), (97, 131), (5000, 2)]      # (W, H)
MODES = [(mode, hmv) for mode in (ref.FIXED16, ref.ROUNDED) for hmv in (0, 1)]
SENT_U8, SENT_F = 0xA5, np.float32(-777.25)


@pytest.fixture(scope="module")
def pkg():
    import torch                         # torch first: it brings its own HIP runtime and must initialise before ours
    assert torch.cuda.is_available(), "the -m gpu suite needs an MI355X"
    return load()


def q_simple(W, H):
    """the Q of test_depth_stats_device_matches_oracle, centred on the frame: h_3 = d / 2.4, so d = 0 divides by zero"""
    return np.array([[1, 0, 0, -(W / 2 + 0.5)], [0, 1, 0, -(H / 2 + 0.25)], [0, 0, 0, 310.7], [0, 0, 1 / 2.4, 0.0]])


def q_full(W, H):
    """all 16 entries non-zero; h_3 = ... + d / 2.4 - 5.3 changes sign where d passes about 12.7"""
    return np.array([[1.01, 0.02, 0.03, -(W / 2 + 0.5)], [0.015, 0.99, -0.02, -(H / 2 + 0.25)],
                     [0.001, -0.002, 0.004, 310.7], [0.0007, -0.0003, 1 / 2.4, -5.3]])


def random_disp(rng, n, W, H, invalid_share, dmax=32, floor=0):
    """n x H x W int16 x16 maps: values in [floor * 16, dmax * 16) and the invalid marker -16 on about invalid_share"""
    d = rng.integers(floor * 16, dmax * 16, (n, H, W)).astype(np.int16)
    d[rng.random((n, H, W)) < invalid_share] = -16
    return d


def random_guide_mask(rng, n, W, H, cn=3, mask_share=0.7):
    g = rng.integers(0, 256, (n, H, W, cn) if cn == 3 else (n, H, W)).astype(np.uint8) if cn else None
    m = ((rng.random((n, H, W)) < mask_share) * rng.integers(1, 256, (n, H, W))).astype(np.uint8)
    return g, m


def padded(torch, a, sentinel, pad_rows=1, pad_cols=3):
    """a device copy of the n x H x W [x c] array `a` as a view of a larger, sentinel-filled tensor: row pitch and frame
    stride exceed the frame.  Returns (whole tensor, view)."""
    t = torch.from_numpy(np.ascontiguousarray(a))
    shape = list(a.shape)
    shape[1] += pad_rows; shape[2] += pad_cols
    whole = torch.full(shape, sentinel, dtype=t.dtype, device="cuda")
    view = whole[:, :a.shape[1], :a.shape[2]]
    view.copy_(t)
    return whole, view


def guards_untouched(whole, H, W, sentinel):
    w = whole.cpu().numpy().copy()
    w[:, :H, :W] = sentinel
    return bool((w == sentinel).all())


def device_run(pkg, rp, disp, guide=None, mask=None, capacity=None, want_map=True, want_cloud=True):
    """Runs map_device and cloud_device on a stream of the test's own, with pitched, guarded planes.
    -> dict(xyz, z: n x H x W [x 3] arrays; pts: list of POINT arrays; counts; raw: the n x bytes point buffer)"""
    import torch
    n, H, W = disp.shape
    _, d_disp = padded(torch, disp, -16)
    d_guide = padded(torch, guide, 0)[1] if guide is not None else None
    d_mask = padded(torch, mask, 0)[1] if mask is not None else None
    out = {}
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    if want_map:
        xyz_whole = torch.full((n, H + 1, W + 2, 3), float(SENT_F), dtype=torch.float32, device="cuda")
        z_whole = torch.full((n, H + 2, W + 5), float(SENT_F), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        rp.map_device(d_disp, xyz_whole[:, :H, :W], z_whole[:, :H, :W], stream=st.cuda_stream)
        st.synchronize()
        assert guards_untouched(xyz_whole, H, W, SENT_F) and guards_untouched(z_whole, H, W, SENT_F)
        out["xyz"] = xyz_whole[:, :H, :W].cpu().numpy()
        out["z"] = z_whole[:, :H, :W].cpu().numpy()
    if want_cloud:
        cap = W * H if capacity is None else capacity
        pts_whole = torch.full((n, cap * 16 + 48), SENT_U8, dtype=torch.uint8, device="cuda")
        counts = torch.full((n + 1,), -12345, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        rp.cloud_device(d_disp, pts_whole[:, :cap * 16], counts[:n], d_guide=d_guide, d_mask=d_mask, capacity=cap,
                        stream=st.cuda_stream)
        st.synchronize()
        c = counts.cpu().numpy()
        assert c[n] == -12345
        raw = pts_whole.cpu().numpy()
        out["counts"], out["raw"], out["pts"] = c[:n], raw, []
        for i in range(n):
            wr = min(int(c[i]), cap)
            assert (raw[i, wr * 16:] == SENT_U8).all(), "frame %d: bytes beyond record %d were written" % (i, wr)
            out["pts"].append(raw[i, :wr * 16].view(ref.POINT))
    return out


def same_bytes(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


def assert_mixed(disp, Q, mode, hmv, mask=None, min_disparity=0):
    """a random case is one only if the reference keeps some pixels of every frame and drops some"""
    n, H, W = disp.shape
    for i in range(n):
        kept = len(ref.cloud(disp[i], Q, mode, hmv, min_disparity, mask=None if mask is None else mask[i]))
        assert 1 <= kept <= W * H - 1, "frame %d: the reference keeps %d of %d pixels" % (i, kept, W * H)


def check_frames(out, disp, Q, mode, hmv, guide=None, mask=None, capacity=None, min_disparity=0, max_z=1e4):
    n = disp.shape[0]
    for i in range(n):
        if "xyz" in out:
            want = ref.reproject(disp[i], Q, mode, hmv)
            bad = np.argwhere(~((out["xyz"][i] == want) | (np.isnan(out["xyz"][i]) & np.isnan(want))))
            assert len(bad) == 0, "frame %d: xyz differs at %d entries, first (y, x, c) = %s: %r, want %r" % (
                i, len(bad), tuple(bad[0]), out["xyz"][i][tuple(bad[0])], want[tuple(bad[0])])
            assert np.array_equal(out["xyz"][i], want, equal_nan=True)
            assert np.array_equal(out["z"][i], want[..., 2], equal_nan=True)
        if "pts" in out:
            want = ref.cloud(disp[i], Q, mode, hmv, min_disparity, max_z, None if guide is None else guide[i],
                             None if mask is None else mask[i])
            assert int(out["counts"][i]) == len(want), "frame %d: count %d, want %d" % (i, out["counts"][i], len(want))
            cap = len(want) if capacity is None else capacity
            assert same_bytes(out["pts"][i], want[:cap]), "frame %d: records differ" % i


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("W,H", SHAPES)
def test_every_shape_mode_and_matrix(pkg, W, H, n):
    rng = np.random.default_rng(1000 * W + 10 * H + n)
    disp = random_disp(rng, n, W, H, 0.3 if W * H > 1 else 0.0)
    guide, mask = random_guide_mask(rng, n, W, H)
    rp = pkg.HIPReprojector(q_simple(W, H), W, H, max_batch=2)
    try:
        for Q in (q_simple(W, H), q_full(W, H)):
            if Q[3, 3] != 0 and W * H >= 64:       # the sign change of h_3 is inside the frame
                z = ref.reproject(disp[0], Q, ref.FIXED16, False)[..., 2]
                assert (z < 0).any() and (z > 0).any()
            for mode, hmv in MODES:
                if W * H >= 64:                    # smaller frames are edge cases, not random ones
                    assert_mixed(disp, Q, mode, hmv, mask)
                rp.set_params(Q=Q, disparity_mode=mode, handle_missing_values=hmv)
                check_frames(device_run(pkg, rp, disp, guide, mask), disp, Q, mode, hmv, guide, mask)
    finally:
        rp.close()


@pytest.mark.parametrize("share", [0.01, 0.5, 0.99])
def test_kept_shares(pkg, share):
    W, H, n = 97, 131, 3
    rng = np.random.default_rng(int(share * 100))
    disp = random_disp(rng, n, W, H, 1.0 - share, floor=1)
    Q = q_simple(W, H)
    for i in range(n):
        kept = len(ref.cloud(disp[i], Q, ref.ROUNDED, True))
        assert 1 <= kept <= W * H - 1
        assert abs(kept / (W * H) - share) < 0.05
    rp = pkg.HIPReprojector(Q, W, H, max_batch=2)
    try:
        check_frames(device_run(pkg, rp, disp), disp, Q, ref.ROUNDED, True)
    finally:
        rp.close()


def test_edge_contents(pkg):
    W, H = 257, 5
    Q = q_simple(W, H)
    rng = np.random.default_rng(7)
    rp = pkg.HIPReprojector(Q, W, H, max_batch=2)
    try:
        # all invalid: count 0, nothing written (device_run asserts the untouched bytes)
        d = np.full((1, H, W), -16, np.int16)
        out = device_run(pkg, rp, d)
        assert out["counts"][0] == 0 and len(out["pts"][0]) == 0
        check_frames(out, d, Q, ref.ROUNDED, True)
        # only the last pixel kept
        d[0, H - 1, W - 1] = 160
        out = device_run(pkg, rp, d)
        assert out["counts"][0] == 1
        check_frames(out, d, Q, ref.ROUNDED, True)
        # all kept: count = W * H = capacity (no missing-value handling, every Z finite and below max_z)
        d = random_disp(rng, 1, W, H, 0.0, floor=1)
        rp.set_params(handle_missing_values=0)
        out = device_run(pkg, rp, d)
        assert out["counts"][0] == W * H
        check_frames(out, d, Q, ref.ROUNDED, False)
        # no invalid marker in the frame: X4 removes the valid pixels at the minimum
        rp.set_params(handle_missing_values=1)
        out = device_run(pkg, rp, d)
        at_min = int((ref.disparity(d[0], ref.ROUNDED) == ref.disparity(d[0], ref.ROUNDED).min()).sum())
        assert at_min >= 1 and out["counts"][0] == W * H - at_min
        check_frames(out, d, Q, ref.ROUNDED, True)
        # frames of one batch with different minima, in both modes
        d = np.stack([random_disp(rng, 1, W, H, 0.0, floor=f)[0] for f in (3, 9, 1)])
        assert len({int(x.min()) for x in d}) == 3
        for mode in (ref.FIXED16, ref.ROUNDED):
            rp.set_params(disparity_mode=mode)
            check_frames(device_run(pkg, rp, d), d, Q, mode, True)
    finally:
        rp.close()


@pytest.mark.parametrize("min_disparity", [-4, 3])
def test_negative_sub_pixel_disparities_and_the_matchers_marker(pkg, min_disparity):
    """Raw values below zero (a matcher with minDisparity < 0): the rounding of negative ties, the rounded zero -- +0.0, as
    the reference's integer map has it, where h_3's other terms are -0.0 and the sign of the zero picks +inf or -inf -- and
    X6's marker (min_disparity - 1) * 16 at a value other than -16."""
    W, H, n = 257, 5, 3
    marker = (min_disparity - 1) * 16
    rng = np.random.default_rng(40 + min_disparity)
    disp = rng.integers(min_disparity * 16, (min_disparity + 12) * 16, (n, H, W)).astype(np.int16)
    disp[rng.random((n, H, W)) < 0.3] = marker
    disp[:, 0, :16] = np.arange(-16, 0)                # every raw value whose rounded quotient is -1, -0 or 0, at x, y from 0
    Q = np.array([[1, 0, 0, -128.5], [0, 1, 0, -2.25], [0, 0, 0, 310.7], [-0.0, -0.0, 1 / 2.4, -0.0]])
    zero = (ref.disparity(disp[0], ref.ROUNDED) == 0) & (disp[0] < 0)
    assert zero.sum() >= 8 and (ref.reproject(disp[0], Q, ref.ROUNDED, False)[..., 2][zero] == np.inf).all()
    rp = pkg.HIPReprojector(Q, W, H, min_disparity=min_disparity, max_batch=2)
    try:
        for mode, hmv in MODES:
            assert_mixed(disp, Q, mode, hmv, None, min_disparity)
            rp.set_params(disparity_mode=mode, handle_missing_values=hmv)
            out = device_run(pkg, rp, disp)
            check_frames(out, disp, Q, mode, hmv, min_disparity=min_disparity)
            if not hmv:                                # the marker is dropped by X6 itself, not by X4
                finite = np.isfinite(ref.reproject(disp[0], Q, mode, False)[..., 2]) & (disp[0] == marker)
                assert finite.any() and out["counts"][0] <= W * H - int((disp[0] == marker).sum())
    finally:
        rp.close()


@pytest.mark.parametrize("n", [1, 3])
def test_capacity_below_the_count(pkg, n):
    W, H = 2049, 3
    Q = q_full(W, H)
    rng = np.random.default_rng(11 + n)
    disp = random_disp(rng, n, W, H, 0.2)
    guide, _ = random_guide_mask(rng, n, W, H)
    rp = pkg.HIPReprojector(Q, W, H, mode=pkg.XYZ_FIXED16, max_batch=2)
    try:
        full = [len(ref.cloud(disp[i], Q, ref.FIXED16, True)) for i in range(n)]
        for cap in (0, 1, 1000, 1025, min(full) - 1):        # inside a tile, at a tile's first record, one short
            assert cap < min(full)
            out = device_run(pkg, rp, disp, guide, None, capacity=cap, want_map=False)
            assert [int(c) for c in out["counts"]] == full       # reported in full
            check_frames(out, disp, Q, ref.FIXED16, True, guide, None, capacity=cap)
            # the host entry: the same records, and the caller's array is not touched beyond them
            pts, cnt = rp.cloud(disp[0], guide=guide[0], capacity=cap)
            assert cnt == full[0] and same_bytes(pts, ref.cloud(disp[0], Q, ref.FIXED16, True, guide=guide[0])[:cap])
    finally:
        rp.close()


def test_host_cloud_leaves_the_bytes_after_the_records(pkg):
    W, H = 65, 2
    Q = q_simple(W, H)
    disp = random_disp(np.random.default_rng(3), 1, W, H, 0.5)[0]
    want = ref.cloud(disp, Q)
    assert 2 <= len(want) < W * H
    B = pkg.binding
    rp = pkg.HIPReprojector(Q, W, H)
    try:
        for cap in (len(want) - 1, W * H):
            buf = np.full(W * H * 16 + 16, SENT_U8, np.uint8)
            cnt = C.c_int()
            B.check(B.lib().rtdm_xyz_cloud(rp._h, disp.ctypes.data, W * 2, None, 0, 0, None, 0, W, H, buf.ctypes.data, cap,
                                           C.byref(cnt)), "rtdm_xyz_cloud")
            wr = min(cap, len(want))
            assert cnt.value == len(want) and buf[:wr * 16].tobytes() == want[:wr].tobytes() and (buf[wr * 16:] == SENT_U8).all()
    finally:
        rp.close()


@pytest.mark.parametrize("with_mask", [False, True])
@pytest.mark.parametrize("cn", [0, 1, 3])
def test_guide_and_mask(pkg, cn, with_mask):
    W, H, n = 97, 131, 3
    Q = q_simple(W, H)
    rng = np.random.default_rng(20 + cn)
    disp = random_disp(rng, n, W, H, 0.4)
    guide, mask = random_guide_mask(rng, n, W, H, cn)
    mask = mask if with_mask else None
    assert_mixed(disp, Q, ref.ROUNDED, True, mask)
    rp = pkg.HIPReprojector(Q, W, H, max_batch=2)
    try:
        out = device_run(pkg, rp, disp, guide, mask, want_map=False)
        check_frames(out, disp, Q, ref.ROUNDED, True, guide, mask)
        if cn == 0:
            assert not out["pts"][0]["r"].any() and (out["pts"][0]["a"] == 255).all()
        # the host entry, with planes that are views of wider arrays
        wide = np.zeros((H, W + 9), np.int16)
        wide[:, :W] = disp[0]
        pts, cnt = rp.cloud(wide[:, :W], guide=None if guide is None else guide[0], mask=None if mask is None else mask[0])
        want = ref.cloud(disp[0], Q, guide=None if guide is None else guide[0], mask=None if mask is None else mask[0])
        assert cnt == len(want) and same_bytes(pts, want)
    finally:
        rp.close()


@pytest.fixture(scope="module")
def pair(pkg, oracle):
    s = pkg.synth
    L, R = s.make_pair(s.STREAM_SEED + 78, 320, 240, 32)
    return L, R, oracle.bm_compute(L, R, numDisparities=32, blockSize=9)


QS = np.array([[1, 0, 0, -160.5], [0, 1, 0, -120.25], [0, 0, 0, 310.7], [0, 0, 1 / 2.4, 0.0]])


def test_host_map_and_depth(pkg, pair):
    _, _, d = pair
    wide = np.zeros((240, 333), np.int16)
    wide[:, :320] = d
    for mode, hmv in MODES:
        rp = pkg.HIPReprojector(QS, 320, 240, mode=mode, handleMissingValues=bool(hmv))
        try:
            want = ref.reproject(d, QS, mode, hmv)
            assert np.array_equal(rp.reprojectImageTo3D(wide[:, :320]), want, equal_nan=True)
            assert np.array_equal(rp.depth(d), want[..., 2], equal_nan=True)
        finally:
            rp.close()
    assert np.isinf(want[..., 2]).any()          # d = 0 divides by h_3 = 0


def test_cloud_agrees_with_depth_stats_device(pkg, pair):
    import torch
    L, _, d = pair
    mask = ((L > 110) * 255).astype(np.uint8)
    regions = [(40, 30, 100, 80), (0, 0, 320, 240), (317, 200, 3, 40)]
    mean, cnt = pkg.depth_stats_device(torch.from_numpy(d).cuda(), QS, torch.from_numpy(mask).cuda(), regions)
    rp = pkg.HIPReprojector(QS, 320, 240)        # ROUNDED, missing values handled, max_z 1e4: the reference's call
    try:
        for (x, y, w, h), m, c in zip(regions, mean, cnt):
            inside = np.zeros_like(mask)
            inside[y:y + h, x:x + w] = mask[y:y + h, x:x + w]
            pts, count = rp.cloud(d, mask=inside)
            assert count == int(c)
            s = 0.0
            for z in pts["z"]:
                s += float(z)
            got = (s / count) * 25.0 / 10.0 if count else 0.0
            assert got == pytest.approx(m, rel=1e-9, abs=0)
    finally:
        rp.close()


def test_pipeline_from_the_matcher(pkg, pair):
    L, R, d = pair
    mask = ((L > 110) * 255).astype(np.uint8)
    guide = np.stack([L, R, 255 - L], axis=2)
    m = pkg.HIPMatcher(numOfDisparities=32, blockSize=9, width=320, height=240)
    rp = pkg.HIPReprojector(QS, 320, 240, min_disparity=0, mode=pkg.XYZ_FIXED16)
    try:
        pts, cnt, disp = rp.compute(m, L, R, guide=guide, mask=mask, want_disp=True)
        assert np.array_equal(disp, d)
        want = ref.cloud(d, QS, ref.FIXED16, True, guide=guide, mask=mask)
        assert cnt == len(want) and same_bytes(pts, want)
        pts, cnt = rp.compute(m, L, R, capacity=100)
        assert cnt == 55433 and same_bytes(pts, ref.cloud(d, QS, ref.FIXED16, True)[:100])
        other = pkg.HIPReprojector(QS, 320, 240, min_disparity=4)
        try:
            with pytest.raises(pkg.binding.RtdmError) as e:    # min_disparity must be the matcher's
                other.compute(m, L, R)
            assert e.value.status == -1
        finally:
            other.close()
    finally:
        rp.close()
        m.close()


def test_two_runs_give_identical_bytes(pkg):
    W, H, n = 5000, 2, 3
    Q = q_full(W, H)
    rng = np.random.default_rng(5)
    disp = random_disp(rng, n, W, H, 0.5)
    guide, mask = random_guide_mask(rng, n, W, H)
    assert_mixed(disp, Q, ref.ROUNDED, True, mask)
    rp = pkg.HIPReprojector(Q, W, H, max_batch=2)
    try:
        a = device_run(pkg, rp, disp, guide, mask)
        b = device_run(pkg, rp, disp, guide, mask)
        assert a["xyz"].tobytes() == b["xyz"].tobytes() and a["z"].tobytes() == b["z"].tobytes()
        assert a["raw"].tobytes() == b["raw"].tobytes() and a["counts"].tobytes() == b["counts"].tobytes()
    finally:
        rp.close()


def test_statuses_with_a_live_handle(pkg):
    B = pkg.binding
    L = B.lib()
    W, H = 64, 8
    rp = pkg.HIPReprojector(q_simple(W, H), W, H)
    try:
        d = np.zeros((H, W), np.int16)
        g = np.zeros((H, W, 3), np.uint8)
        out = np.zeros((H, W, 3), np.float32)
        pts = np.zeros(W * H, ref.POINT)
        cnt = C.c_int()
        dp, gp, op, pp = d.ctypes.data, g.ctypes.data, out.ctypes.data, pts.ctypes.data
        assert L.rtdm_xyz_map(rp._h, dp, W * 2, W, H, None, 0, None, 0) == -2             # both outputs absent
        assert L.rtdm_xyz_map(rp._h, dp, W * 2 - 2, W, H, op, W * 12, None, 0) == -2      # pitch smaller than a row
        assert L.rtdm_xyz_map(rp._h, dp, W * 2, W, H, op, W * 12 - 4, None, 0) == -2
        assert L.rtdm_xyz_map(rp._h, dp, W * 2, W + 1, H, op, W * 12 + 12, None, 0) == -2   # beyond the handle's frame
        assert L.rtdm_xyz_map(rp._h, None, W * 2, W, H, op, W * 12, None, 0) == -7
        assert L.rtdm_xyz_cloud(rp._h, dp, W * 2, gp, W * 2, 2, None, 0, W, H, pp, W * H, C.byref(cnt)) == -1    # channels
        assert L.rtdm_xyz_cloud(rp._h, dp, W * 2, None, 0, 0, None, 0, W, H, pp, -1, C.byref(cnt)) == -1         # capacity
        assert L.rtdm_xyz_cloud(rp._h, dp, W * 2, None, 0, 3, None, 0, W, H, pp, 4, C.byref(cnt)) == -7          # guide missing
        assert L.rtdm_xyz_cloud(rp._h, dp, W * 2, gp, W * 3 - 1, 3, None, 0, W, H, pp, 4, C.byref(cnt)) == -2
        assert L.rtdm_xyz_cloud(rp._h, dp, W * 2, None, 0, 0, None, 0, W, H, pp, 4, None) == -7
        with pytest.raises(pkg.binding.RtdmError) as e:
            rp.set_params(disparity_mode=3)
        assert e.value.status == -1 and rp.params.disparity_mode == pkg.XYZ_ROUNDED
        with pytest.raises(ValueError):
            rp.cloud(d, capacity=-1)
        with pytest.raises(ValueError):
            rp.cloud(d.astype(np.float32))
        with pytest.raises(ValueError):
            rp.cloud(d, guide=np.zeros((H, W, 2), np.uint8))
        got = B.XYZParams()
        assert L.rtdm_xyz_get_params(rp._h, C.byref(got)) == 0 and got.max_z == 1e4 and got.handle_missing_values == 1
    finally:
        rp.close()
