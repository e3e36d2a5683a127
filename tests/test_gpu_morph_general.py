"""GPU parity of the general morphology path (k_morph_general.hip) against the numpy reference tests/morph_ref.py, through
rtdm_morph_run / rtdm_morph_run_device, rtdm_objects_detect and rtdm_estimate_frame.  Tolerance 0 everywhere.

Frames sit in pitched buffers whose base is 1-3 bytes off a dword and whose bytes outside the frames are guard bands that a
call must leave untouched; batches hold more frames than the handle's max_batch.  The cases and their inputs come from
tests/morph_cases.py: every frame of every case (gray and mask, every operation and iteration count) is chosen so that
the REFERENCE result is neither constant nor the input, and the tests assert that; the only cases without the assertion
are the single erosions / dilations for which the geometry makes it impossible (morph_cases.forced).
tests/test_morph_general_cpu.py walks the same list without a device."""
import numpy as np
import pytest

import golden_util as gu
import morph_cases as mc
import morph_ref as mr
import rectify_util as ru

pytestmark = pytest.mark.gpu

@pytest.fixture(scope="module")
def pkg():
    import torch                         # torch first: it brings its own HIP runtime and must initialise before ours
    assert torch.cuda.is_available()
    from conftest import load
    return load()


def check_nontrivial(want, frame, what):
    assert mc.nontrivial(want, frame), ("the reference result is trivial", what)


def run_case(pkg, mf, c, inplace=False, seed=0):
    """One case of tests/morph_cases.py on a handle whose setting is the case's; every frame is compared."""
    assert mf.get_op()[0] == c["op"] and np.array_equal(mf.get_op()[1], c["el"]) and mf.get_op()[2] == c["it"]
    got = run_device(pkg, mf, c["frames"], inplace=inplace, seed=seed)
    what = (c["W"], c["H"], np.asarray(c["el"]).shape, c["anchor"], c["op"], c["it"], inplace)
    for i, (f, want) in enumerate(zip(c["frames"], c["want"])):
        if c["asserted"][i]:
            check_nontrivial(want, f, what + (i,))
        assert np.array_equal(got[i], want), what + (i,)


def run_device(pkg, mf, frames, inplace=False, seed=0):
    """frames: n arrays H x W -> n results, through pitched, misaligned device buffers with guard bands"""
    import torch
    n, (H, W) = len(frames), frames[0].shape
    rng = np.random.default_rng(seed)
    ioff, ooff = 1 + seed % 3, 1 + (seed + 1) % 3
    ipitch, opitch = W + 5, W + (5 if inplace else 3)
    ifr, ofr = ipitch * H + 7, opitch * H + (7 if inplace else 2)
    src = rng.integers(0, 256, ioff + n * ifr + 8, dtype=np.uint8)
    rows = (np.arange(n)[:, None, None] * ifr + np.arange(H)[None, :, None] * ipitch + np.arange(W)[None, None, :])
    src[ioff + rows] = np.stack(frames)
    d_in = torch.from_numpy(src).cuda()
    if inplace:
        d_out, ooff, dst0, orow = d_in, ioff, src.copy(), rows
    else:
        dst0 = rng.integers(0, 256, ooff + n * ofr + 8, dtype=np.uint8)
        d_out = torch.from_numpy(dst0).cuda()
        orow = (np.arange(n)[:, None, None] * ofr + np.arange(H)[None, :, None] * opitch + np.arange(W)[None, None, :])
    B = pkg.binding
    B.check(B.lib().rtdm_morph_run_device(mf._h, n, d_in.data_ptr() + ioff, ipitch, ifr, d_out.data_ptr() + ooff,
                                          opitch if not inplace else ipitch, ofr if not inplace else ifr, W, H,
                                          torch.cuda.current_stream().cuda_stream), "rtdm_morph_run_device")
    torch.cuda.synchronize()
    got = d_out.cpu().numpy()
    guard = np.ones(got.size, bool)
    guard[ooff + orow] = False
    assert np.array_equal(got[guard], dst0[guard]), "bytes outside the frames were written"
    if not inplace:
        assert np.array_equal(d_in.cpu().numpy(), src), "the input was written"
    return got[ooff + orow]


@pytest.mark.parametrize("shape,w,h", mc.NAMED)
def test_named_elements_on_every_frame(pkg, shape, w, h):
    handles = {}
    for c in mc.named_cases(shape, w, h):
        key = (c["W"], c["H"])
        if key not in handles:
            handles[key] = pkg.HIPMorphologicalFilter(c["W"], c["H"], 8, max_batch=2)       # three frames: two chunks
        mf = handles[key]
        mf.set_op(c["op"], (shape, (w, h)))
        assert mf.get_op()[3] == (w // 2, h // 2)
        run_case(pkg, mf, c, seed=w + h + c["op"])
    for mf in handles.values():
        mf.close()


@pytest.mark.parametrize("seed", range(6))
def test_random_masks_and_corner_anchors(pkg, seed):
    # several runs per row, empty rows and columns at the rim, the anchor in each corner and somewhere inside
    w, h = mc.RANDOM_SIZES[seed]
    el = mr.random_element(w, h, seed)
    assert (np.diff(np.concatenate([[0], el[h // 2].astype(np.int8)])) == 1).sum() >= (2 if w > 3 else 1)
    handles = {}
    for c in mc.random_cases(seed):
        key = (c["W"], c["H"])
        if key not in handles:
            handles[key] = pkg.HIPMorphologicalFilter(c["W"], c["H"], 8, max_batch=1)       # two frames: two chunks
        mf = handles[key]
        mf.set_op(c["op"], c["el"], anchor=c["anchor"])
        assert mf.get_op()[3] == c["anchor"]
        run_case(pkg, mf, c, seed=seed + c["op"])
    for mf in handles.values():
        mf.close()


@pytest.mark.parametrize("op", mr.OPS)
@pytest.mark.parametrize("inplace", [False, True])
def test_every_operation_and_iteration_count(pkg, op, inplace):
    handles = {}
    for c in mc.op_cases(op):
        key = (c["W"], c["H"])
        if key not in handles:
            handles[key] = pkg.HIPMorphologicalFilter(c["W"], c["H"], 8, max_batch=2)
        mf = handles[key]
        mf.set_op(op, c["el"], iterations=c["it"], anchor=c["anchor"])
        assert all(c["asserted"])
        run_case(pkg, mf, c, inplace=inplace, seed=c["it"])
    for mf in handles.values():
        mf.close()


@pytest.mark.parametrize("op", mr.OPS)
@pytest.mark.parametrize("inplace", [False, True])
def test_aligned_frames_take_the_dword_paths(pkg, op, inplace):
    # dense 16-byte aligned tensors whose width is a multiple of 4: interior tiles are staged by dwords, results and the
    # second input of a difference go by dwords (what a 1280-wide frame does); 260 columns leave a partial tile at the right
    import torch
    handles = {}
    for c in mc.aligned_cases(op):
        key = (c["W"], c["H"])
        if key not in handles:
            handles[key] = pkg.HIPMorphologicalFilter(c["W"], c["H"], 8, max_batch=2)
        mf = handles[key]
        mf.set_op(op, c["el"], anchor=c["anchor"])
        d_in = torch.from_numpy(np.stack(c["frames"])).cuda()
        d_out = d_in if inplace else torch.empty_like(d_in)
        assert d_in.data_ptr() % 16 == 0 and d_out.data_ptr() % 16 == 0 and all(c["asserted"])
        mf.run_device(d_in, d_out, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        got = d_out.cpu().numpy()
        for i in range(3):
            check_nontrivial(c["want"][i], c["frames"][i], (c["W"], c["H"], op, i))
            assert np.array_equal(got[i], c["want"][i]), (c["W"], c["H"], np.asarray(c["el"]).shape, op, inplace, i)
    for mf in handles.values():
        mf.close()


def test_set_op_between_calls_on_a_live_handle(pkg):
    W, H = 97, 65
    gray = mr.gray_frame(W, H, 40)
    mf = pkg.HIPMorphologicalFilter(W, H, 8)
    op, el, it, anchor = mf.get_op()
    assert (op, it, anchor) == (pkg.MORPH_OPEN_CLOSE, 1, (5, 5)) and np.array_equal(el, mr.element(mr.ELLIPSE, 10, 10))
    first = mf.run(gray)
    wants = [mr.morphology(gray, mr.OPEN_CLOSE, el), mr.morphology(gray, mr.GRADIENT, mr.element(mr.CROSS, 5, 9), None, 2),
             mr.morphology(gray, mr.TOPHAT, np.ones((4, 63), bool), (62, 3))]
    for i, want in enumerate(wants):
        check_nontrivial(want, gray, ("set_op", i))
    assert np.array_equal(first, wants[0])
    mf.set_op(pkg.MORPH_GRADIENT, (pkg.MORPH_CROSS, (5, 9)), iterations=2)
    assert np.array_equal(mf.run(gray), wants[1])
    mf.set_op(pkg.MORPH_TOPHAT, np.ones((4, 63), np.uint8), anchor=(62, 3))
    assert np.array_equal(mf.run(gray), wants[2])
    with pytest.raises(pkg.binding.RtdmError) as e:                              # a refused setting leaves the last one
        mf.set_op(7, (pkg.MORPH_RECT, (3, 3)))
    assert e.value.status == -1 and mf.get_op()[0] == pkg.MORPH_TOPHAT
    mf.set_op(pkg.MORPH_OPEN_CLOSE)                                              # back to the default
    assert np.array_equal(mf.run(gray), first)
    mf.close()


def test_default_setting_on_the_general_path(pkg):
    # the switch is process wide: the default handle then runs k_morph_pass four times instead of k_morph_open_close
    L = pkg.binding.lib()
    W, H = 233, 156
    el = mr.element(mr.ELLIPSE, 10, 10)
    gray, mask = (mc.pick(kind, W, H, el, None, mr.OPEN_CLOSE, 1, seed)[0] for kind, seed in (("gray", 50), ("mask", 51)))
    mf = pkg.HIPMorphologicalFilter(W, H, 8)
    fused = [mf.run(gray), mf.run(mask)]
    L.rtdm_debug_morph_general(1)
    try:
        assert np.array_equal(mf.run(gray), fused[0]) and np.array_equal(mf.run(mask), fused[1])
        check_nontrivial(fused[0], gray, "default, gray")
        check_nontrivial(fused[1], mask, "default, mask")
        assert np.array_equal(fused[0], mr.morphology(gray, mr.OPEN_CLOSE, el)) and np.array_equal(fused[1], mr.morphology(mask, mr.OPEN_CLOSE, el))
        for name in gu.morph_cases():
            z = gu.load_morph(name)
            h, w = z["mask"].shape
            g = pkg.HIPMorphologicalFilter(w, h, 8)
            assert np.array_equal(g.run(z["mask"]), z["mask_out"]), name
            assert np.array_equal(g.run(z["gray"]), z["gray_out"]), name
            g.close()
    finally:
        L.rtdm_debug_morph_general(0)
    mf.close()


def paint(mask, rng):
    """RGB crop whose red filter response is exactly `mask` (as tests/test_gpu_objects.py)."""
    H, W = mask.shape
    g = rng.integers(0, 256, (H, W), dtype=np.uint8)
    rgb = np.stack([g, g, g], -1)
    rgb[mask] = np.stack([150 + g.astype(np.int32) // 3, g // 6, g // 6], -1).astype(np.uint8)[mask]
    return np.ascontiguousarray(rgb)


@pytest.mark.parametrize("setting", ["rect5", "random"])
def test_detector_with_another_filter(pkg, oracle, setting):
    W, H = 233, 156
    rng = np.random.default_rng(60)
    rgb = paint(mr.mask_frame(W, H, 61) != 0, rng)
    el, anchor = (mr.element(mr.RECT, 5, 5), None) if setting == "rect5" else (mr.random_element(7, 5, 62), (1, 3))
    det = pkg.HIPObjectDetector(W, H)
    assert det.get_op()[0] == pkg.MORPH_OPEN_CLOSE and np.array_equal(det.get_op()[1], mr.element(mr.ELLIPSE, 10, 10))
    det.set_op(pkg.MORPH_OPEN_CLOSE, el, anchor=anchor)
    m = oracle.hsv_inrange(rgb, oracle.HSV_LOW, oracle.HSV_HIGH)
    want_out = mr.morphology(m, mr.OPEN_CLOSE, el, anchor)
    check_nontrivial(want_out, m, setting)
    assert not np.array_equal(want_out, oracle.morph_open_close(m))              # the setting matters
    for zb in (True, False):
        boxes, roi, out = det.detect(rgb, min_area=20, zero_border=zb, max_boxes=1024)
        want = oracle.external_boxes(np.ascontiguousarray(want_out), 20, zb)
        assert np.array_equal(out, want_out) and boxes == want and len(want) >= 1, (setting, zb)
        assert roi == oracle.union_box(want)
    det.close()


def test_whole_frame_chain_with_a_reconfigured_detector(pkg, oracle, synth):
    # the chain of tests/test_gpu_objects.py::test_whole_frame_chain, the detector filtering with ELLIPSE 13x13
    # (smaller elements leave the scene's objects joined into one box)
    res, D, w, min_area = "320x240", 32, 7, 40
    c, maps = ru.maps(oracle, res)
    left, right = ru.red_scene(synth, 1, c["W"], c["H"], D)
    x, y, rw, rh = c["roi"]
    rect = pkg.HIPRectifier(*maps, roi=c["roi"])
    m = pkg.HIPMatcher(numOfDisparities=D, blockSize=w, width=rw, height=rh)
    det = pkg.HIPObjectDetector(rw, rh)
    el = mr.element(mr.ELLIPSE, 13, 13)
    det.set_op(pkg.MORPH_OPEN_CLOSE, (pkg.MORPH_ELLIPSE, (13, 13)))
    boxes, mean, cnt, disp = pkg.estimate_frame(m, rect, det, left, right, c["Q"], min_area=min_area, want_disp=True)
    gl = oracle.rectify_gray(left, maps[0], maps[1], c["roi"]); gr = oracle.rectify_gray(right, maps[2], maps[3], c["roi"])
    col = oracle.rectify_rgb(left, maps[0], maps[1], c["roi"])
    fout = np.ascontiguousarray(mr.morphology(oracle.hsv_inrange(col, oracle.HSV_LOW, oracle.HSV_HIGH), mr.OPEN_CLOSE, el))
    want_boxes = oracle.external_boxes(fout, min_area, True)
    assert len(want_boxes) >= 2 and boxes == want_boxes[:64]
    want_disp = oracle.bm_compute(gl, gr, numDisparities=D, blockSize=w, roi1=oracle.union_box(want_boxes), nthreads=8)
    assert np.array_equal(disp, want_disp)
    wm, wc = oracle.depth_stats(want_disp, c["Q"], fout, want_boxes[:64])
    assert np.array_equal(cnt, wc) and wc.sum() > 0
    assert np.allclose(mean, wm, rtol=1e-9, atol=0)
    det.close(); m.close(); rect.close()


def test_cpp_adapter_core_sets_element_and_operation(tmp_path):
    # HIPMorphCore::setElement / setOperation, what HIPMorphologicalFilter of host/mf-hip.cpp forwards to
    import subprocess
    from test_morph_general_cpu import build_core_program
    out = subprocess.run([build_core_program(tmp_path), "gpu"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "bad shape: -1\n" in out.stdout and "bad size: -1\n" in out.stdout and "large: -6\n" in out.stdout
    assert "set: 0 0\n" in out.stdout and "hitmiss: -1 iterations: -1\n" in out.stdout and "close: equal, changed: yes" in out.stdout
