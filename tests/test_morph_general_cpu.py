"""No-GPU checks of the general morphology path: the element maker of the C ABI against the numpy reference (tests/morph_ref.py)
and the oracle, the reference itself against the oracle, the stored goldens and scipy, and every refusal of
rtdm_morph_set_op / rtdm_objects_set_morph / rtdm_morph_make_element, which are decided before a device is needed."""
import ctypes as C
import os

import numpy as np
import pytest

import golden_util as gu
import morph_cases as mc
import morph_ref as mr
from conftest import load

ELLIPSES = [(10, 10), (3, 3), (7, 4), (5, 11), (31, 31), (2, 2), (1, 9), (9, 1), (63, 63)]


@pytest.fixture(scope="module")
def B():
    return load("binding")


@pytest.fixture(scope="module")
def noise():
    return np.random.default_rng(5).integers(0, 256, (72, 97), dtype=np.uint8)


def c_element(B, shape, w, h):
    el = B.MorphElement()
    assert B.lib().rtdm_morph_make_element(shape, w, h, C.byref(el)) == 0, (shape, w, h)
    assert (el.width, el.height, el.anchor_x, el.anchor_y) == (w, h, w // 2, h // 2)
    return np.frombuffer(el.mask, np.uint8, w * h).reshape(h, w) != 0


def test_make_element_equals_the_reference_at_every_size(B, oracle):
    for w in range(1, 64):
        for h in range(1, 64):
            for shape in (mr.RECT, mr.CROSS, mr.ELLIPSE):
                assert np.array_equal(c_element(B, shape, w, h), mr.element(shape, w, h)), (shape, w, h)
            assert np.array_equal(mr.element(mr.ELLIPSE, w, h), oracle.ellipse_element(w, h) != 0), (w, h)


def test_element_quirks(B):
    pkg = load()
    assert c_element(B, mr.ELLIPSE, 9, 1).sum() == 1                       # a single pixel
    assert c_element(B, mr.ELLIPSE, 1, 9).sum() == 9                       # a column
    e = pkg.get_structuring_element(pkg.MORPH_ELLIPSE, (10, 10))
    assert e.dtype == bool and e.shape == (10, 10) and not np.array_equal(e, e[::-1])      # even sizes are asymmetric
    assert [int(r.sum()) for r in e] == [1, 7, 9, 10, 10, 10, 10, 10, 9, 7]
    assert c_element(B, mr.CROSS, 1, 1).all() and c_element(B, mr.ELLIPSE, 1, 1).all()
    with pytest.raises(pkg.binding.RtdmError):
        pkg.get_structuring_element(3, (5, 5))
    with pytest.raises(ValueError):
        pkg.get_structuring_element(pkg.MORPH_RECT, 5)


@pytest.mark.parametrize("kw,kh", ELLIPSES)
def test_reference_equals_the_oracle(oracle, noise, kw, kh):
    el = mr.element(mr.ELLIPSE, kw, kh)
    assert np.array_equal(mr.erode(noise, el), oracle.erode(noise, kw, kh))
    assert np.array_equal(mr.dilate(noise, el), oracle.dilate(noise, kw, kh))


@pytest.mark.parametrize("name", gu.morph_cases())
def test_reference_reproduces_the_goldens(name):
    z = gu.load_morph(name)
    el = mr.element(mr.ELLIPSE, 10, 10)
    assert np.array_equal(mr.morphology(z["mask"], mr.OPEN_CLOSE, el), z["mask_out"])
    assert np.array_equal(mr.morphology(z["gray"], mr.OPEN_CLOSE, el), z["gray_out"])


@pytest.mark.parametrize("shape", [mr.RECT, mr.CROSS, mr.ELLIPSE])
def test_reference_equals_scipy(noise, shape):
    from scipy import ndimage as ndi
    for w, h in ELLIPSES + [(63, 2), (4, 6)]:
        el = mr.element(shape, w, h)
        # scipy centres the footprint at size // 2 too (origin 0), and does not reflect it for either filter
        assert np.array_equal(mr.erode(noise, el), ndi.minimum_filter(noise, footprint=el, mode="constant", cval=255)), (w, h)
        assert np.array_equal(mr.dilate(noise, el), ndi.maximum_filter(noise, footprint=el, mode="constant", cval=0)), (w, h)


def _walk(cases):
    frames = asserted = 0
    for c in cases:                                                        # pick() raises where a case has no usable input
        for f, want, must in zip(c["frames"], c["want"], c["asserted"]):
            frames += 1
            asserted += must
            assert must == mc.nontrivial(want, f)
            if not must:                                                   # only where the geometry forces it, for both kinds of pass
                assert c["op"] in (mr.ERODE, mr.DILATE) and c["it"] == 1 and mc.forced(c["W"], c["H"], c["el"], c["anchor"])
    return frames, asserted


@pytest.mark.parametrize("shape", [mr.RECT, mr.CROSS, mr.ELLIPSE])
def test_gpu_named_cases_have_nontrivial_inputs(shape):
    # the GPU tests' own case list (tests/morph_cases.py): every frame of every case has a reference result that is neither
    # constant nor the input, except the single passes whose geometry makes that impossible
    frames = asserted = 0
    for s, w, h in mc.NAMED:
        if s == shape:
            n, a = _walk(mc.named_cases(s, w, h))
            frames, asserted = frames + n, asserted + a
    assert frames == 10 * 7 * 2 * 3 and 0 < asserted < frames          # some geometries are forced: the 1x1 frame, the 1x1 element


def test_gpu_random_cases_have_nontrivial_inputs():
    for seed in range(6):
        frames, asserted = _walk(mc.random_cases(seed))
        assert frames == 3 * 5 * 2 * 2 and asserted == frames, seed


@pytest.mark.parametrize("op", mr.OPS)
def test_gpu_operation_cases_have_nontrivial_inputs(op):
    for gen in (mc.op_cases, mc.aligned_cases):
        frames, asserted = _walk(gen(op))
        assert frames > 0 and asserted == frames


def test_forced_geometry_is_what_it_says():
    # the exclusion rule against brute force: every input of a forced geometry gives a constant or the input itself
    rng = np.random.default_rng(3)
    for W, H, el, forced in ((5, 3, mr.element(mr.ELLIPSE, 63, 63), True), (5, 3, mr.element(mr.CROSS, 63, 63), False),
                             (63, 1, mr.element(mr.RECT, 1, 9), True), (63, 1, mr.element(mr.ELLIPSE, 9, 1), True),
                             (1, 1, mr.element(mr.RECT, 3, 3), True), (64, 32, mr.element(mr.RECT, 63, 63), False),
                             (5, 3, mr.element(mr.RECT, 63, 2), False), (5, 3, mr.element(mr.RECT, 10, 10), True), (5, 3, mr.element(mr.RECT, 3, 3), False)):
        assert mc.forced(W, H, el, None) == forced, (W, H, el.shape)
        if forced:
            for _ in range(20):
                f = rng.integers(0, 256, (H, W), dtype=np.uint8)
                assert not mc.nontrivial(mr.erode(f, el), f) and not mc.nontrivial(mr.dilate(f, el), f)


def hand_element(B, w, h, ax, ay, fill=1):
    el = B.MorphElement(w, h, ax, ay)
    for i in range(max(w, 0) * max(h, 0) if w <= 63 and h <= 63 else 0):
        el.mask[i] = fill
    return el


@pytest.mark.parametrize("setter", ["rtdm_morph_set_op", "rtdm_objects_set_morph"])
def test_refusals_need_no_device(B, setter):
    L = B.lib()
    fn = getattr(L, setter)
    ok = hand_element(B, 5, 5, 2, 2)
    BAD, UNS, NUL = -1, -6, -7
    # values are judged before the handle: a NULL handle never hides them
    for op in (-1, 7, 8, 99, 101):                                         # 7 = cv::MORPH_HITMISS
        assert fn(None, op, 1, C.byref(ok)) == BAD, op
    for it in (0, -1, 17):
        assert fn(None, B.MORPH_ERODE, it, C.byref(ok)) == BAD, it
    for w, h in ((0, 5), (5, 0), (-1, 3)):
        assert fn(None, B.MORPH_ERODE, 1, C.byref(hand_element(B, w, h, 0, 0))) == BAD, (w, h)
    for ax, ay in ((-1, 2), (5, 2), (2, -1), (2, 5)):
        assert fn(None, B.MORPH_ERODE, 1, C.byref(hand_element(B, 5, 5, ax, ay))) == BAD, (ax, ay)
    assert fn(None, B.MORPH_ERODE, 1, C.byref(hand_element(B, 5, 5, 2, 2, fill=0))) == BAD          # all-zero mask
    for w, h in ((64, 5), (5, 64), (200, 200)):
        assert fn(None, B.MORPH_ERODE, 1, C.byref(hand_element(B, w, h, 1, 1))) == UNS, (w, h)
    assert fn(None, B.MORPH_ERODE, 1, None) == NUL
    for op in list(range(7)) + [B.MORPH_OPEN_CLOSE]:                       # all is well but the handle
        for it in (1, 16):
            assert fn(None, op, it, C.byref(ok)) == NUL, (op, it)
    getter = L.rtdm_morph_get_op if setter == "rtdm_morph_set_op" else L.rtdm_objects_get_morph
    assert getter(None, None, None, None) == NUL


def test_make_element_refusals_and_abi_version(B):
    L = B.lib()
    el = B.MorphElement()
    assert L.rtdm_morph_make_element(B.MORPH_RECT, 3, 3, None) == -7
    for shape in (-1, 3, 7):
        assert L.rtdm_morph_make_element(shape, 3, 3, C.byref(el)) == -1
    for w, h in ((0, 3), (3, 0), (-2, -2)):
        assert L.rtdm_morph_make_element(B.MORPH_RECT, w, h, C.byref(el)) == -1
    for w, h in ((64, 3), (3, 64)):
        assert L.rtdm_morph_make_element(B.MORPH_ELLIPSE, w, h, C.byref(el)) == -6
    assert L.rtdm_morph_make_element(B.MORPH_ELLIPSE, 63, 63, C.byref(el)) == 0
    assert L.rtdm_abi_version() == 3
    L.rtdm_debug_morph_general(1)                                          # a switch, not a device call
    L.rtdm_debug_morph_general(0)
    assert C.sizeof(B.MorphElement) == 16 + 63 * 63 + 3                    # four ints, the mask, padding to 4


def test_python_argument_checks_raise():
    pkg = load()
    M = load("morph")
    with pytest.raises(ValueError):
        M._morph_element(np.zeros((0, 3)), None)
    with pytest.raises(ValueError):
        M._morph_element(np.ones(5), None)
    with pytest.raises(pkg.binding.RtdmError) as e:
        M._morph_element(np.ones((64, 3)), None)
    assert e.value.status == -6
    with pytest.raises(ValueError):
        M._morph_element((pkg.MORPH_RECT, (3, 3)), anchor=1)
    el = M._morph_element([[0, 1, 1], [1, 0, 2]], (2, 1))
    assert (el.width, el.height, el.anchor_x, el.anchor_y) == (3, 2, 2, 1) and list(el.mask[:6]) == [0, 1, 1, 1, 0, 1]
    el = M._morph_element(None, None)
    assert (el.width, el.height, el.anchor_x, el.anchor_y) == (10, 10, 5, 5)
    assert (pkg.MORPH_RECT, pkg.MORPH_CROSS, pkg.MORPH_ELLIPSE) == (0, 1, 2)
    assert [pkg.MORPH_ERODE, pkg.MORPH_DILATE, pkg.MORPH_OPEN, pkg.MORPH_CLOSE, pkg.MORPH_GRADIENT, pkg.MORPH_TOPHAT,
            pkg.MORPH_BLACKHAT, pkg.MORPH_OPEN_CLOSE] == list(mr.OPS)


def test_adapter_declares_the_setters():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    h = open(os.path.join(root, "rt-depth-map_amd", "host", "mf-hip.h")).read()
    assert "int setElement(int shape, int width, int height);" in h and "int setOperation(int op, int iterations = 1);" in h
    assert "explicit HIPMorphologicalFilter(int w, int h, int bpp);" in h


def build_core_program(tmp_path):
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkgdir = os.path.join(root, "rt-depth-map_amd")
    exe = str(tmp_path / "morph_core_host")
    subprocess.check_call(["g++", "-O1", "-std=c++11", "-Wall", "-Werror", "-I", os.path.join(pkgdir, "host"),
                           os.path.join(root, "tests", "morph_core_host.cpp"), "-L", os.path.join(pkgdir, "lib"), "-lrtdm_host",
                           "-lrtdm_hip", "-Wl,-rpath," + os.path.join(pkgdir, "lib"), "-o", exe])
    return exe


def test_adapter_core_element_refusals_compile_and_link(tmp_path):
    # the program itself is run by the GPU test: its first act is to create a handle.  Here: it builds against the adapter's
    # header and libraries, and the refusals it prints are those of rtdm_morph_make_element, which needs no device
    build_core_program(tmp_path)
    L = load("binding").lib()
    el = load("binding").MorphElement()
    assert [L.rtdm_morph_make_element(*a, C.byref(el)) for a in ((3, 5, 5), (0, 0, 5), (0, 64, 5))] == [-1, -1, -6]


def test_run_table_builder_under_the_host_sanitizers(tmp_path):
    # morph_element_bits (csrc/rtdm_kernels.h) in a stand-alone program of its own: AddressSanitizer + UBSan on HOST code
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "morph_bits_host")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Xarch_host", "-fsanitize=address,undefined",
                           "-Xarch_host", "-fno-sanitize-recover=all", "-I", os.path.join(root, "rt-depth-map_amd", "csrc"),
                           os.path.join(root, "tests", "morph_bits_host.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.startswith("ok: 0 failed checks over 11907 masks"), run.stdout + run.stderr
