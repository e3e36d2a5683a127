"""The one download of rtdm_bm's internal disparity plane that four host entry points share (bm_download_disp /
bm_scatter_disp, api_bm.hip), where it can go wrong: a frame of 157 x 113, whose internal rows are Ws = 160 elements, into a
caller's plane with a row pitch of 2 * 157 + 10 bytes.  rtdm_bm_compute_depth, rtdm_bm_compute_rgb, rtdm_estimate_frame and
rtdm_bm_compute_mjpeg must each give, bit for bit, what the same steps give through rtdm_bm_compute (which keeps its own
two-band download), leave the bytes between 2 * W and the pitch alone, and do so again with freshly created handles."""
import ctypes as C

import numpy as np
import pytest

import mjpeg_synth as mj
import rectify_util as ru
from conftest import load

pytestmark = pytest.mark.gpu

W, H, D, BLOCK = 157, 113, 32, 9
SW, SH, ROI = 160, 120, (1, 3, W, H)           # source frames; identity maps, so the crop is the rectified frame
PITCH, SENTINEL = 2 * W + 10, 0xA5
ROUTES = ("depth", "rgb", "estimate", "mjpeg")


def _stream(rgb):
    """a 4:2:2 baseline frame of the image, built by tests/mjpeg_synth.py"""
    q = [np.full(64, 3, np.int64), np.full(64, 5, np.int64)]
    comps = [mj.into_domain(b, k) for b, k in zip(mj.blocks_from_image(rgb, [q[0], q[1], q[1]], "2x1"), [q[0], q[1], q[1]])]
    return mj.write(SW, SH, "2x1", comps, {0: q[0], 1: q[1]}, ri=5)


def _cycle(pkg, frames, streams):
    """create the four handles, take every route once, destroy them -> {route: (got rows, want rows, padding untouched)}"""
    B = load("binding")
    lib = B.lib()
    yy, xx = np.mgrid[0:SH, 0:SW]
    m1, m2 = np.ascontiguousarray(np.stack([xx, yy], -1).astype(np.int16)), np.zeros((SH, SW), np.uint16)
    rect = pkg.HIPRectifier(m1, m2, m1, m2, ROI)
    bm = pkg.HIPMatcher(numOfDisparities=D, blockSize=BLOCK, width=W, height=H)
    det = pkg.HIPObjectDetector(W, H)
    dec = pkg.HIPMJPEGDecoder(SW, SH, max_stream_bytes=max(len(s) for s in streams))
    out = {}

    def pitched(call):
        buf = np.full((H, PITCH), SENTINEL, np.uint8)
        call(buf.ctypes.data)
        return buf[:, :2 * W].copy().view(np.int16), bool((buf[:, 2 * W:] == SENTINEL).all())

    try:
        left, right = frames
        gl, gr = rect.gray(left, right)
        q = np.eye(4).reshape(16)
        qp = q.ctypes.data_as(C.POINTER(C.c_double))
        mask = np.full((H, W), 255, np.uint8)
        reg, mean, cnt = (B.Region * 1)(B.Region(0, 0, W, H)), (C.c_double * 64)(), (C.c_int * 64)()
        got = pitched(lambda p: B.check(lib.rtdm_bm_compute_depth(
            bm._h, gl.ctypes.data, gl.strides[0], gr.ctypes.data, gr.strides[0], W, H, qp, mask.ctypes.data, W, reg, 1, 25.0,
            mean, cnt, p, PITCH), "rtdm_bm_compute_depth"))
        out["depth"] = got + (bm.compute(gl, gr),)
        got = pitched(lambda p: B.check(lib.rtdm_bm_compute_rgb(
            bm._h, rect._h, left.ctypes.data, left.strides[0], right.ctypes.data, right.strides[0], p, PITCH), "rtdm_bm_compute_rgb"))
        out["rgb"] = got + (bm.compute(gl, gr),)
        dl, dr = dec.decode(streams[0]), dec.decode(streams[1])
        got = pitched(lambda p: B.check(lib.rtdm_bm_compute_mjpeg(
            bm._h, rect._h, dec._h, streams[0], len(streams[0]), streams[1], len(streams[1]), SW, SH, p, PITCH), "rtdm_bm_compute_mjpeg"))
        out["mjpeg"] = got + (rect.compute(bm, dl, dr),)
        # last: the call leaves ROI 1 of the matcher set to the union of its boxes
        boxes, n = (B.Region * 64)(), C.c_int()
        rng = B.HsvRange((C.c_int * 3)(*pkg.objects.HSV_LOW), (C.c_int * 3)(*pkg.objects.HSV_HIGH))
        got = pitched(lambda p: B.check(lib.rtdm_estimate_frame(
            bm._h, rect._h, det._h, left.ctypes.data, left.strides[0], right.ctypes.data, right.strides[0], qp, C.byref(rng), 40, 1,
            25.0, boxes, mean, cnt, 64, C.byref(n), p, PITCH), "rtdm_estimate_frame"))
        assert 1 <= n.value <= 64
        bx = [(b.x, b.y, b.x + b.width, b.y + b.height) for b in boxes[:n.value]]
        x0, y0, x1, y1 = min(b[0] for b in bx), min(b[1] for b in bx), max(b[2] for b in bx), max(b[3] for b in bx)
        bm.setROI1((x0, y0, x1 - x0, y1 - y0))
        out["estimate"] = got + (bm.compute(gl, gr),)
    finally:
        dec.close(); det.close(); bm.close(); rect.close()
    return out


@pytest.fixture(scope="module")
def cycles(synth):
    import torch                         # torch first: it brings its own HIP runtime and must initialise before ours
    assert torch.cuda.is_available()
    pkg = load()
    frames = ru.red_scene(synth, 1, SW, SH, D)
    streams = [_stream(f) for f in frames]
    return [_cycle(pkg, frames, streams) for _ in range(2)]


@pytest.mark.parametrize("route", ROUTES)
def test_shared_download_equals_the_matcher_entry_point(cycles, route):
    got, intact, want = cycles[0][route]
    assert want.shape == (H, W) and (want != (0 - 1) * 16).mean() > 0.05        # a map with content, not all FILTERED
    assert np.array_equal(got, want)
    assert intact


@pytest.mark.parametrize("route", ROUTES)
def test_a_second_set_of_handles_gives_the_same_planes(cycles, route):
    again, intact, want = cycles[1][route]
    assert np.array_equal(again, cycles[0][route][0]) and np.array_equal(want, cycles[0][route][2]) and intact
