"""The host entry points whose row staging goes through rtdm::copy_rows (csrc/rtdm_rows.h), called through the raw C ABI on
fixed seeded inputs in two layouts, and the device-form calls that give the same results from frames uploaded by torch.

Layouts.  `dense`: every plane contiguous.  `view`: every plane is a view that starts at byte X0 > 0 of the rows of a parent
buffer with an odd pitch (an even one where the ABI asks for it) and padded frame strides; the parent ENDS with the view's last
row, so the byte behind the last pixel is outside the allocation's used part.  All parent bytes outside a view hold PAD; take()
checks that a call left them alone.

tests/test_gpu_host_staging.py asserts on what run_host / run_device return; profiles/host_staging_hashes.txt is the
SHA-256 listing of run_host's arrays (hash_lines) on the parent of the change that introduced copy_rows and on that change."""
import ctypes as C
import hashlib
import importlib

import numpy as np

import estimate_batch_scenes as sc
import rectify_util as ru

D, BLOCK, MIN_AREA, CAP, NFRAMES, CHUNK = 32, 9, 40, 16, 3, 2
SIZES = ((157, 113), (157, 257), (160, 113))      # internal rows of 160; one band / two bands, odd split; no pad columns
PAD, X0 = 0xA5, 6
REGIONS = [(10, 8, 60, 50), (70, 40, 80, 60), (0, 0, 157, 113)]
RED = ((0, 150, 0), (9, 255, 255))
RANGES = [RED, (sc.BLUE_LOW, sc.BLUE_HIGH)]


class Buf:
    """`frames` planes of rows x row_bytes bytes in one of the two layouts; `fill`: the planes' content (any dtype)."""

    def __init__(self, rows, row_bytes, view, fill=None, frames=1, even=False, pinned=False):
        self.shape = (frames, rows, row_bytes)
        self.x0 = X0 if view else 0
        self.pitch = (((row_bytes + 13) | 1) + (1 if even else 0)) if view else row_bytes
        self.stride = self.pitch * rows + 18 if view else row_bytes * rows
        n = self.x0 + (frames - 1) * self.stride + (rows - 1) * self.pitch + row_bytes
        if pinned:
            import torch
            self._keep = torch.empty(n, dtype=torch.uint8).pin_memory()
            self.flat = self._keep.numpy()
        else:
            self.flat = np.empty(n, np.uint8)
        self.flat[:] = PAD
        self.ptr = self.flat.ctypes.data + self.x0
        if fill is not None:
            self._planes(self.flat)[...] = np.ascontiguousarray(fill).view(np.uint8).reshape(self.shape)

    def _planes(self, flat):
        return np.lib.stride_tricks.as_strided(flat[self.x0:], self.shape, (self.stride, self.pitch, 1))

    def take(self, dtype, shape):
        outside = np.ones(self.flat.size, bool)
        self._planes(outside)[...] = False
        assert (self.flat[outside] == PAD).all(), "bytes outside the view were written"
        return np.ascontiguousarray(self._planes(self.flat)).view(dtype).reshape(shape)


class Rig:
    """Inputs and handles for W x H frames (rectified from W + 23 x H + 20 sensor frames with constant sub-pixel maps)."""

    def __init__(self, pkg, W, H):
        self.pkg, self.W, self.H = pkg, W, H
        self.lib = pkg.binding.lib()
        self.marshal = importlib.import_module(pkg.__name__ + "._marshal")
        synth = pkg.synth
        self.L, self.R = synth.make_pair(synth.STREAM_SEED + 31, W, H, D)
        self.L3, self.R3 = ru.rgb_pair(synth, 3, W, H)
        self.mask = np.where(self.L > 100, 255, 0).astype(np.uint8)
        self.Q = ru.calib("320x240")["Q"]
        self.SW, self.SH, self.roi = W + 23, H + 20, (11, 9, W, H)
        scenes = [sc.two_colour_scene(synth, {"W": self.SW, "H": self.SH}, seed) for seed in (1, 2, 3)]
        self.lefts = np.stack([s[0] for s in scenes]); self.rights = np.stack([s[1] for s in scenes])
        yy, xx = np.mgrid[0:self.SH, 0:self.SW]
        map1 = np.ascontiguousarray(np.stack([xx, yy], -1).astype(np.int16))
        map2 = np.full((self.SH, self.SW), 9 * 32 + 9, np.uint16)          # the same sub-pixel shift everywhere, in both cameras
        self.m = pkg.HIPMatcher(numOfDisparities=D, blockSize=BLOCK, width=W, height=H)
        self.me = pkg.HIPMatcher(numOfDisparities=D, blockSize=BLOCK, width=W, height=H, max_batch=CHUNK)   # (estimates set its ROI1)
        self.sg = pkg.HIPSemiGlobalMatcher(numOfDisparities=D, width=W, height=H, paths=5)
        self.mf = pkg.HIPMorphologicalFilter(W, H, 8)
        self.rect = pkg.HIPRectifier(map1, map2, map1, map2, roi=self.roi, max_batch=CHUNK)
        self.det = pkg.HIPObjectDetector(W, H, max_batch=CHUNK, max_classes=2)
        self.est = pkg.HIPEstimator(self.me, self.rect, self.det, max_batch=CHUNK, capacity=CAP)
        self.crop = self.rect.rgb(self.lefts[0])           # the detector's input: the rectified colour crop of the first scene

    def close(self):
        for h in (self.est, self.det, self.rect, self.mf, self.sg, self.me, self.m):
            h.close()


def _ok(status, where):
    assert status == 0, "%s returned %d" % (where, status)


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


def run_host(r, view):
    """Every host entry point once -> {"call.array": ndarray}."""
    lib, W, H, SW, SH, pkg = r.lib, r.W, r.H, r.SW, r.SH, r.pkg
    q = r.marshal.q16(r.Q)
    out = {}

    def gray(pinned=False):
        return Buf(H, W, view, r.L, pinned=pinned), Buf(H, W, view, r.R, pinned=pinned), Buf(H, 2 * W, view, pinned=pinned)

    def sensor(f=0):
        return Buf(SH, 3 * SW, view, r.lefts[f]), Buf(SH, 3 * SW, view, r.rights[f])

    for name, pinned in (("bm_compute", False), ("bm_compute_page_locked", True)):
        a, b, o = gray(pinned)
        _ok(lib.rtdm_bm_compute(r.m._h, a.ptr, a.pitch, b.ptr, b.pitch, W, H, o.ptr, o.pitch), name)
        out[name + ".disp"] = o.take(np.int16, (H, W))

    regions = [(x, y, min(w, W - x), min(h, H - y)) for x, y, w, h in REGIONS]
    for name, want in (("bm_compute_depth", True), ("bm_compute_depth_no_disp", False)):
        a, b, o = gray()
        k = Buf(H, W, view, r.mask)
        mean = np.full(len(regions), -7.0); cnt = np.full(len(regions), -7, np.int32)
        _ok(lib.rtdm_bm_compute_depth(r.m._h, a.ptr, a.pitch, b.ptr, b.pitch, W, H, q, k.ptr, k.pitch, r.marshal.regions_array(regions),
                                      len(regions), 25.0, _dp(mean), _ip(cnt), o.ptr if want else None, o.pitch), name)
        out[name + ".mean"], out[name + ".counts"] = mean, cnt
        disp = o.take(np.int16, (H, W))
        if want:
            out[name + ".disp"] = disp
        else:
            assert (disp.view(np.uint8) == PAD).all()

    a, b = sensor()
    gl, gr = Buf(H, W, view), Buf(H, W, view)
    _ok(lib.rtdm_rectify_gray(r.rect._h, a.ptr, a.pitch, b.ptr, b.pitch, gl.ptr, gl.pitch, gr.ptr, gr.pitch), "rectify_gray")
    out["rectify_gray.left"], out["rectify_gray.right"] = gl.take(np.uint8, (H, W)), gr.take(np.uint8, (H, W))
    for which in (0, 1):
        o = Buf(H, 3 * W, view)
        src = (a, b)[which]
        _ok(lib.rtdm_rectify_rgb(r.rect._h, which, src.ptr, src.pitch, o.ptr, o.pitch), "rectify_rgb")
        out["rectify_rgb.%d" % which] = o.take(np.uint8, (H, W, 3))

    a = Buf(H, 3 * W, view, r.crop)
    o = Buf(H, W, view)
    boxes = (pkg.binding.Region * 64)(); n = C.c_int(); roi = pkg.binding.Region()
    rng = pkg.objects._hsv_range(*RED)
    _ok(lib.rtdm_objects_detect(r.det._h, a.ptr, a.pitch, C.byref(rng), MIN_AREA, 1, o.ptr, o.pitch, boxes, 64, C.byref(n), C.byref(roi)),
        "objects_detect")
    out["objects_detect.boxes"] = np.array([(v.x, v.y, v.width, v.height) for v in boxes[:n.value]], np.int32).reshape(-1, 4)
    out["objects_detect.roi"] = np.array([roi.x, roi.y, roi.width, roi.height], np.int32)
    out["objects_detect.mask"] = o.take(np.uint8, (H, W))

    for cn, (left, right) in ((1, (r.L, r.R)), (3, (r.L3, r.R3))):
        a, b, o = Buf(H, cn * W, view, left), Buf(H, cn * W, view, right), Buf(H, 2 * W, view)
        _ok(lib.rtdm_sgm_compute_cn(r.sg._h, cn, a.ptr, a.pitch, b.ptr, b.pitch, W, H, o.ptr, o.pitch), "sgm_compute_cn")
        out["sgm_compute_cn%d.disp" % cn] = o.take(np.int16, (H, W))

    a, o = Buf(H, W, view, r.mask), Buf(H, W, view)
    _ok(lib.rtdm_morph_run(r.mf._h, a.ptr, a.pitch, o.ptr, o.pitch, W, H), "morph_run")
    out["morph_run.out"] = o.take(np.uint8, (H, W))

    a, b = sensor()
    o = Buf(H, 2 * W, view)
    boxes = (pkg.binding.Region * CAP)(); n = C.c_int()
    mean = np.zeros(CAP); cnt = np.zeros(CAP, np.int32)
    _ok(lib.rtdm_estimate_frame(r.me._h, r.rect._h, r.det._h, a.ptr, a.pitch, b.ptr, b.pitch, q, C.byref(rng), MIN_AREA, 1, 25.0, boxes,
                                _dp(mean), _ip(cnt), CAP, C.byref(n), o.ptr, o.pitch), "estimate_frame")
    k = min(n.value, CAP)
    out["estimate_frame.boxes"] = np.array([(v.x, v.y, v.width, v.height) for v in boxes[:k]], np.int32).reshape(-1, 4)
    out["estimate_frame.mean"], out["estimate_frame.counts"] = mean[:k], cnt[:k]
    out["estimate_frame.disp"] = o.take(np.int16, (H, W))

    o = Buf(H, 2 * W, view)
    objs = np.zeros(CAP, pkg.OBJECT_DTYPE); mean = np.zeros(CAP); cnt = np.zeros(CAP, np.int32)
    crng, ccls, nr, K = pkg.objects._hsv_classes(RANGES, None)
    _ok(lib.rtdm_estimate_frame_classes(r.me._h, r.rect._h, r.det._h, a.ptr, a.pitch, b.ptr, b.pitch, q, crng, ccls, nr, K, MIN_AREA, 1, 25.0,
                                        objs.ctypes.data, _dp(mean), _ip(cnt), CAP, C.byref(n), o.ptr, o.pitch), "estimate_frame_classes")
    k = min(n.value, CAP)
    out["estimate_frame_classes.objects"] = objs[:k].copy().view(np.int32).reshape(k, 8)[:, :6]
    out["estimate_frame_classes.mean"], out["estimate_frame_classes.counts"] = mean[:k], cnt[:k]
    out["estimate_frame_classes.disp"] = o.take(np.int16, (H, W))

    a, b = Buf(SH, 3 * SW, view, r.lefts, NFRAMES), Buf(SH, 3 * SW, view, r.rights, NFRAMES)
    for name, full in (("estimate_batch", False), ("estimate_batch_measured", True)):
        o = Buf(H, 2 * W, view, frames=NFRAMES, even=True)
        objs = np.zeros((NFRAMES, CAP), pkg.OBJECT_DTYPE); counts = np.zeros((NFRAMES, K), np.int32)
        mean = np.zeros((NFRAMES, CAP)); npix = np.zeros((NFRAMES, CAP), np.int32)
        args = (r.est._h, NFRAMES, a.ptr, a.pitch, a.stride, b.ptr, b.pitch, b.stride, q, crng, ccls, nr, K, MIN_AREA, 1, 25.0, objs.ctypes.data,
                counts.ctypes.data, mean.ctypes.data, npix.ctypes.data, o.ptr if full else None, o.pitch, o.stride)
        if full:
            mp = pkg.MeasureParams()
            meas = np.zeros((NFRAMES, CAP), pkg.MEASURE_DTYPE)
            _ok(lib.rtdm_estimate_batch_measured(*(args + (C.byref(mp.c), meas.ctypes.data))), name)
            out[name + ".measures"] = meas.view(np.uint8).reshape(NFRAMES, CAP * 88)
            out[name + ".disp"] = o.take(np.int16, (NFRAMES, H, W))
        else:
            _ok(lib.rtdm_estimate_batch(*args), name)
        out[name + ".objects"] = objs.view(np.int32).reshape(NFRAMES, CAP, 8)[:, :, :6]
        out[name + ".counts"], out[name + ".mean"], out[name + ".npix"] = counts, mean, npix
    return out


def run_device(r):
    """The device-form entry points on the same frames, uploaded by torch -> the arrays of run_host they must equal bit for bit
    (objects_detect.boxes: as a sorted list; the device form lists the objects in its own order)."""
    import torch
    pkg, W, H = r.pkg, r.W, r.H
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731
    out = {}
    d = torch.zeros((1, H, W), dtype=torch.int16, device="cuda")
    r.m.compute_device(dev(r.L[None]), dev(r.R[None]), d)
    out["bm_compute.disp"] = d[0].cpu().numpy()
    gl = torch.zeros((1, H, W), dtype=torch.uint8, device="cuda"); gr = torch.zeros_like(gl)
    r.rect.gray_device(dev(r.lefts[:1]), dev(r.rights[:1]), gl, gr)
    out["rectify_gray.left"], out["rectify_gray.right"] = gl[0].cpu().numpy(), gr[0].cpu().numpy()
    for cn, (left, right) in ((1, (r.L, r.R)), (3, (r.L3, r.R3))):
        d = torch.zeros((1, H, W), dtype=torch.int16, device="cuda")
        r.sg.compute_device(dev(left[None]), dev(right[None]), d)
        out["sgm_compute_cn%d.disp" % cn] = d[0].cpu().numpy()
    o = torch.zeros((1, H, W), dtype=torch.uint8, device="cuda")
    r.mf.run_device(dev(r.mask[None]), o)
    out["morph_run.out"] = o[0].cpu().numpy()
    d_obj = torch.zeros((1, 64 * 32), dtype=torch.uint8, device="cuda"); d_cnt = torch.zeros((1, 1), dtype=torch.int32, device="cuda")
    d_roi = torch.zeros((1, 4), dtype=torch.int32, device="cuda"); d_mask = torch.zeros((1, 1, H, W), dtype=torch.uint8, device="cuda")
    r.det.detect_device(dev(r.crop[None]), [RED], None, d_obj, d_cnt, d_roi, d_mask, min_area=MIN_AREA)
    torch.cuda.synchronize()
    rec = d_obj.cpu().numpy().view(pkg.OBJECT_DTYPE)[0, :int(d_cnt.cpu()[0, 0])]
    out["objects_detect.boxes"] = sorted(zip(rec["x"].tolist(), rec["y"].tolist(), rec["width"].tolist(), rec["height"].tolist()))
    out["objects_detect.roi"], out["objects_detect.mask"] = d_roi[0].cpu().numpy(), d_mask[0, 0].cpu().numpy()
    K = len(RANGES)
    d_obj = torch.zeros((NFRAMES, CAP * 32), dtype=torch.uint8, device="cuda"); d_cnt = torch.zeros((NFRAMES, K), dtype=torch.int32, device="cuda")
    d_mean = torch.zeros((NFRAMES, CAP), dtype=torch.float64, device="cuda"); d_npix = torch.zeros((NFRAMES, CAP), dtype=torch.int32, device="cuda")
    d_disp = torch.full((NFRAMES, H, W), PAD * 257 - 65536, dtype=torch.int16, device="cuda")      # (what an untouched host frame holds)
    d_meas = torch.zeros((NFRAMES, CAP * 88), dtype=torch.uint8, device="cuda")
    r.est.estimate_device(dev(r.lefts), dev(r.rights), r.Q, RANGES, None, d_obj, d_cnt, d_mean, d_npix, d_disp=d_disp, min_area=MIN_AREA,
                          d_measures=d_meas)
    torch.cuda.synchronize()
    objects = d_obj.cpu().numpy().view(np.int32).reshape(NFRAMES, CAP, 8)[:, :, :6]
    for name in ("estimate_batch", "estimate_batch_measured"):
        out[name + ".objects"], out[name + ".counts"] = objects, d_cnt.cpu().numpy()
        out[name + ".mean"], out[name + ".npix"] = d_mean.cpu().numpy(), d_npix.cpu().numpy()
    out["estimate_batch_measured.disp"], out["estimate_batch_measured.measures"] = d_disp.cpu().numpy(), d_meas.cpu().numpy()
    return out


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def hash_lines(W, H, layout, results):
    return ["%dx%d %s %s %s" % (W, H, layout, name, sha(a)) for name, a in sorted(results.items())]
