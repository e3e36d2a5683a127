"""The MJPEG decoder without a GPU: the NumPy rules (mjpeg_ref.py, J1-J5 of DESIGN.md section 4.12) against the images Pillow /
libjpeg-turbo decoded from the stored streams, the host parser (rtdm_mjpeg_probe) and its refusals, the built-in standard
Huffman tables, the host build of the device's segment-decoding loop (coefficients equal the NumPy ones; single-byte damage ends
in bounds under -fsanitize=address,undefined), and the C++ adapter against a stand-in DecoderDevice."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import mjpeg_ref as ref
from conftest import ROOT, load
from mjpeg_hostbuild import build_dump as _build_dump, build_host as _build_host, records as _records

CSRC = os.path.join(ROOT, "rt-depth-map_amd", "csrc")
HOST = os.path.join(ROOT, "rt-depth-map_amd", "host")
OK, BAD_SIZE, NO_DEVICE, UNSUPPORTED, BAD_STREAM = 0, -2, -3, -6, -8

# W, H, components, luma sampling, restart interval, segments, has_dht
GEOMETRY = {
    "mjpeg_16x8_422_q75": (16, 8, 3, 2, 1, 0, 1, 1),
    "mjpeg_1x1_420_q75": (1, 1, 3, 2, 2, 0, 1, 1),
    "mjpeg_33x17_422_q90": (33, 17, 3, 2, 1, 0, 1, 1),
    "mjpeg_50x34_420_q75_rstrows": (50, 34, 3, 2, 2, 4, 3, 1),
    "mjpeg_97x65_422_q75_rst3": (97, 65, 3, 2, 1, 3, 21, 1),
    "mjpeg_40x24_444_q100_noise": (40, 24, 3, 1, 1, 0, 1, 1),
    "mjpeg_64x48_gray_q50_opt": (64, 48, 1, 1, 1, 0, 1, 1),
    "mjpeg_97x65_422_q30_opt": (97, 65, 3, 2, 1, 0, 1, 1),
    "mjpeg_96x64_422_q75_nodht": (96, 64, 3, 2, 1, 0, 1, 0),
    "mjpeg_96x64_422_q75_gradient": (96, 64, 3, 2, 1, 0, 1, 1),
    "mjpeg_33x17_422_q90_corrupt": (33, 17, 3, 2, 1, 0, 1, 1),
    "mjpeg_4x5_420_q90_narrow": (4, 5, 3, 2, 2, 0, 1, 1),
    "mjpeg_264x64_gray_q50_rst1": (264, 64, 1, 1, 1, 1, 264, 1),
    "mjpeg_200x40_422_q60_rst1": (200, 40, 3, 2, 1, 1, 65, 1),
    "mjpeg_137x73_420_q75_rst2": (137, 73, 3, 2, 2, 2, 23, 1),
}
GEOMETRY.update({n: (97, 65, 3, 2, 1, 3, 21, 1) for n in ref.BATCH})


@pytest.fixture(scope="module")
def std():
    return ref.std_tables()


def _probe(stream, length=None):
    B = load("binding")
    info = B.MJPEGInfo()
    buf = bytes(stream)
    st = B.lib().rtdm_mjpeg_probe(buf, len(buf) if length is None else length, C.byref(info))
    return st, info


# ---- the rules against the library ------------------------------------------------------------------------------------------
def test_the_fixtures_are_all_there_within_the_size_limit():
    assert len(ref.FIXTURES) == 20 and sorted(GEOMETRY) == sorted(ref.FIXTURES)
    for n in ref.FIXTURES + ["mjpeg_aux"]:
        assert os.path.getsize(os.path.join(ref.GOLDEN, n + ".npz")) < 48 * 1024, n


@pytest.mark.parametrize("name", ref.FIXTURES)
def test_numpy_rules_reproduce_pillow_exactly(std, name):
    stream, rgb, _ = ref.load_fixture(name)
    got = ref.decode(stream, std)
    assert got.shape == rgb.shape and np.array_equal(got, rgb), "%d bytes differ" % int((got != rgb).sum())


def test_fixtures_exercise_what_they_are_for(std):
    f = ref.parse(ref.load_fixture("mjpeg_97x65_422_q75_rst3")[0], std)
    assert len(f.segments) == 21 and f.ri == 3                            # the RST number wraps past 7
    s = ref.load_fixture("mjpeg_97x65_422_q75_rst3")[0]
    assert b"\xff\xd7" in s and s.count(b"\xff\xd0") >= 2
    f = ref.parse(ref.load_fixture("mjpeg_40x24_444_q100_noise")[0], std)
    assert all((q == 1).all() for q in f.qt.values())                     # unit quantisers
    assert max(np.abs(c).max() for c in ref.coefficients(f)) > 900        # the largest coefficients
    assert ref.parse(ref.load_fixture("mjpeg_97x65_422_q30_opt")[0], std).huff != std     # non-standard tables
    nodht = ref.load_fixture("mjpeg_96x64_422_q75_nodht")[0]
    assert b"\xff\xc4" not in nodht
    # two chroma columns: interpolating them (the general J3 formula) would NOT give the library's image
    narrow, rgb, _ = ref.load_fixture("mjpeg_4x5_420_q90_narrow")
    f = ref.parse(narrow, std)
    planes = [ref.idct(c) for c in ref.coefficients(f)]
    cb, cr = (np.repeat(np.repeat(p[:3, :2].astype(np.int64), 2, 0), 2, 1)[:5, :4] for p in planes[1:])
    assert np.array_equal(ref.colour(planes[0][:5, :4], cb, cr), rgb) and planes[1][0, 0] != planes[1][0, 1]
    g = ref.coefficients(ref.parse(ref.load_fixture("mjpeg_96x64_422_q75_gradient")[0], std))
    assert np.mean([(c != 0).mean() for c in g]) < 0.1                    # long zero runs, early EOB
    # the launch shapes: 264 segments (256 lanes and a second trip), 65 (128 lanes), 23 (64 lanes); more than 256 blocks each
    # (k_mjpeg_idct's second workgroup, with a partial tail); in the 4:2:0 frame Cb starts inside the first workgroup
    shapes = {}
    for n in ("mjpeg_264x64_gray_q50_rst1", "mjpeg_200x40_422_q60_rst1", "mjpeg_137x73_420_q75_rst2"):
        f = ref.parse(ref.load_fixture(n)[0], std)
        luma, chroma = f.mcux * f.hs * f.mcuy * f.vs, f.mcux * f.mcuy
        shapes[n] = (len(f.segments), luma + (f.ncomp - 1) * chroma, luma)
    assert [shapes[n][0] for n in shapes] == [264, 65, 23]
    assert all(256 < v[1] < 512 for v in shapes.values())
    assert shapes["mjpeg_137x73_420_q75_rst2"][2] % 256 != 0 and shapes["mjpeg_137x73_420_q75_rst2"][2] == 180


# ---- the host parser --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ref.FIXTURES)
def test_probe_reports_the_geometry(name):
    st, i = _probe(ref.load_fixture(name)[0])
    assert st == OK
    assert (i.width, i.height, i.components, i.h_samp, i.v_samp, i.restart_interval, i.segments, i.has_dht) == GEOMETRY[name]


def test_probe_skips_app_com_fill_bytes_and_trailing_bytes():
    s = ref.load_fixture("mjpeg_97x65_422_q75_rst3")[0]
    sos = s.index(b"\xff\xda")
    padded = (s[:2] + b"\xff\xe1\x00\x06Exif" + b"\xff\xfe\x00\x05abc" + s[2:sos] + b"\xff\xff\xff" + s[sos + 1:] + b"\x00" * 37 +
              b"\xff\xd8 not a frame")
    st, i = _probe(padded)
    assert st == OK and (i.width, i.height, i.segments) == (97, 65, 21)
    # a fill byte in front of a restart marker, too
    rst = s.index(b"\xff\xd0", sos)
    st, i = _probe(s[:rst] + b"\xff" + s[rst:])
    assert st == OK and i.segments == 21


def test_builtin_tables_are_the_standard_ones(std):
    """the frame without DHT decodes, on the host build, to the coefficients the stored standard tables give; and those tables
    are what the library writes into a non-optimised stream"""
    nodht = ref.load_fixture("mjpeg_96x64_422_q75_nodht")[0]
    full = ref.load_fixture("mjpeg_96x64_422_q75_gradient")[0]
    assert ref.parse(full, None).huff == std                              # Pillow's plain stream carries exactly these
    assert sorted(std) == [(0, 0), (0, 1), (1, 0), (1, 1)]
    assert [sum(std[k][0]) for k in sorted(std)] == [12, 12, 162, 162]
    # the C tables, read back through the header itself: a tiny program prints them as a DHT payload
    exe = _build_dump()
    out = subprocess.run([exe], capture_output=True, check=True).stdout
    assert out == np.load(os.path.join(ref.GOLDEN, "mjpeg_aux.npz"))["std_dht"].tobytes()


def _refusal_inputs():
    s = ref.load_fixture("mjpeg_33x17_422_q90")[0]
    gray = ref.load_fixture("mjpeg_64x48_gray_q50_opt")[0]
    aux = np.load(os.path.join(ref.GOLDEN, "mjpeg_aux.npz"))
    sof, sos, dqt, dht = s.index(b"\xff\xc0"), s.index(b"\xff\xda"), s.index(b"\xff\xdb"), s.index(b"\xff\xc4")

    def patch(b, at, val):
        return b[:at] + bytes([val]) + b[at + 1:]

    two_comp = patch(patch(s, sof + 9, 2), sos + 4, 2)                    # Nf = 2 (the tests stop at the count)
    return [
        ("progressive", aux["progressive"].tobytes(), UNSUPPORTED),
        ("extended (SOF1)", patch(s, sof + 1, 0xC1), UNSUPPORTED),
        ("lossless (SOF3)", patch(s, sof + 1, 0xC3), UNSUPPORTED),
        ("arithmetic (SOF9)", patch(s, sof + 1, 0xC9), UNSUPPORTED),
        ("12-bit samples", patch(s, sof + 4, 12), UNSUPPORTED),
        ("16-bit quantisers", patch(s, dqt + 4, 0x10), UNSUPPORTED),
        ("two components", two_comp, UNSUPPORTED),
        ("4:1:1 sampling", patch(s, sof + 11, 0x41), UNSUPPORTED),
        ("4:4:0 sampling", patch(s, sof + 11, 0x12), UNSUPPORTED),
        ("chroma sampled 2x1", patch(s, sof + 14, 0x21), UNSUPPORTED),
        ("more than one scan", s[:-2] + s[sos:], UNSUPPORTED),
        ("a scan of one component of three", patch(s, sos + 4, 1), UNSUPPORTED),
        ("no SOI at offset 0", b"\x00" + s, BAD_STREAM),
        ("SOI only", s[:2], BAD_STREAM),
        ("a segment that runs past len", s[:dht + 40], BAD_STREAM),
        ("truncated inside the scan", s[:sos + 40], BAD_STREAM),
        ("no EOI", s[:-2], BAD_STREAM),
        ("no SOS", s[:sos] + b"\xff\xd9", BAD_STREAM),
        ("scan names a missing quantiser", patch(s, sof + 12, 3), BAD_STREAM),
        ("scan names a missing Huffman table", patch(s, sos + 6, 0x22), BAD_STREAM),
        ("gray scan names a missing Huffman table", patch(gray, gray.index(b"\xff\xda") + 6, 0x11), BAD_STREAM),
        ("a restart marker without DRI", s[:sos + 30].replace(b"\xff", b"\x00", 0) + b"\xff\xd0" + s[sos + 30:], BAD_STREAM),
    ]


@pytest.mark.parametrize("case", range(22))
def test_probe_refuses(case):
    what, stream, want = _refusal_inputs()[case]
    st, _ = _probe(stream)
    assert st == want, what


def test_len_is_a_buffer_size_and_bounds_the_parser():
    s = ref.load_fixture("mjpeg_33x17_422_q90")[0]
    buf = s + b"\xff" * 64
    assert _probe(buf)[0] == OK
    for cut in range(0, len(s) - 1, 7):                                   # every prefix is refused, none is read past
        assert _probe(buf, length=cut)[0] == BAD_STREAM, cut
    B = load("binding")
    assert B.lib().rtdm_mjpeg_probe(None, 10, C.byref(B.MJPEGInfo())) == -7
    assert B.lib().rtdm_mjpeg_probe(s, len(s), None) == -7


# ---- handles, binding, ABI --------------------------------------------------------------------------------------------------
def test_create_without_a_device_fails_loudly():
    import torch
    B = load("binding")
    h = C.c_void_p()
    assert B.lib().rtdm_mjpeg_create(0, 48, 1, 4096, 0, C.byref(h)) == BAD_SIZE
    assert B.lib().rtdm_mjpeg_create(64, 48, 1, 0, 0, C.byref(h)) == BAD_SIZE
    assert B.lib().rtdm_mjpeg_create(64, 48, 1, 4096, 0, None) == -7
    st = B.lib().rtdm_mjpeg_create(64, 48, 1, 4096, 0, C.byref(h))
    if torch.cuda.is_available():
        assert st == OK and h.value
        B.lib().rtdm_mjpeg_destroy(h)
        return
    assert st == NO_DEVICE and not h.value
    pkg = load()
    with pytest.raises(B.RtdmError) as e:
        pkg.HIPMJPEGDecoder(64, 48)
    assert e.value.status == NO_DEVICE


def test_new_status_and_exports():
    import re
    B = load("binding")
    L = B.lib()
    assert L.rtdm_abi_version() == 3
    assert B.STATUS[-8] == "RTDM_ERR_BAD_STREAM" and b"JPEG" in L.rtdm_strerror(-8)
    text = open(os.path.join(ROOT, "include", "rtdm.h")).read()
    assert re.search(r"RTDM_ERR_BAD_STREAM\s*=\s*-8", text)
    for n in ("rtdm_mjpeg_probe", "rtdm_mjpeg_create", "rtdm_mjpeg_destroy", "rtdm_mjpeg_decode", "rtdm_mjpeg_decode_batch_device",
              "rtdm_bm_compute_mjpeg"):
        assert n in B.EXPORTS and re.search(r"\b%s\s*\(" % n, text) and hasattr(L, n), n
    assert "rtdm_synth_pairs_device" in B.EXPORTS
    pkg = load()
    assert pkg.mjpeg_probe(ref.load_fixture("mjpeg_16x8_422_q75")[0])["width"] == 16
    with pytest.raises(B.RtdmError) as e:
        pkg.mjpeg_probe(b"\xff\xd8\xff")
    assert e.value.status == BAD_STREAM


# ---- the segment-decoding loop on the CPU -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ref.FIXTURES)
def test_host_build_gives_the_numpy_coefficients(std, tmp_path, name):
    stream = ref.load_fixture(name)[0]
    (tmp_path / "s.jpg").write_bytes(stream)
    subprocess.check_call([_build_host(False), str(tmp_path / "s.jpg"), str(tmp_path / "o.bin")])
    (pst, dst, coef), = _records(str(tmp_path / "o.bin"), 1)
    want = np.concatenate([c.reshape(-1) for c in ref.coefficients(ref.parse(stream, std))])
    assert (pst, dst) == (OK, OK)
    assert np.array_equal(coef.astype(np.int64), want)


def test_single_byte_damage_ends_in_bounds_with_a_status(std, tmp_path):
    """64 seeded single-byte corruptions of the 33x17 stream through the sanitized host build: no report from the address or
    undefined-behaviour sanitizer (either aborts the run), a status of 0 or -8 each, and -8 wherever the NumPy decoder meets a
    bit pattern that is no code or an index past 63.  The eight stored corruptions are among the 64."""
    stream, _, z = ref.load_fixture("mjpeg_33x17_422_q90_corrupt")
    todo = ref.corruptions(stream, ref.CORRUPT_SEED, ref.CORRUPT_COUNT)
    stored = list(zip(z["corrupt_pos"].tolist(), z["corrupt_val"].tolist()))
    assert len(stored) == 8 and all(c in todo for c in stored)
    (tmp_path / "s.jpg").write_bytes(stream)
    args = [str(v) for c in todo for v in c]
    run = subprocess.run([_build_host(True), str(tmp_path / "s.jpg"), str(tmp_path / "o.bin"), *args], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-3000:]
    recs = _records(str(tmp_path / "o.bin"), len(todo))
    verdicts = set()
    for (pos, val), (pst, dst, coef) in zip(todo, recs):
        assert pst == OK and dst in (OK, BAD_STREAM), (pos, val, pst, dst)
        try:
            want = np.concatenate([c.reshape(-1) for c in ref.coefficients(ref.parse(ref.corrupted(stream, pos, val), std))])
        except ValueError:
            assert dst == BAD_STREAM, (pos, val)
            verdicts.add("refused")
            continue
        verdicts.add("accepted" if dst == OK else "overrun")
        if dst == OK:                                 # damage that still parses decodes to the same (wrong) coefficients
            assert np.array_equal(coef.astype(np.int64), np.clip(want, -32768, 32767)), (pos, val)
    assert {"refused", "accepted"} <= verdicts
    sv = {dst for c, (_, dst, _) in zip(todo, recs) if c in stored}
    assert sv == {OK, BAD_STREAM}                     # the GPU meets both kinds


def test_sanitized_host_build_on_every_fixture(tmp_path):
    for name in ref.FIXTURES:
        (tmp_path / "s.jpg").write_bytes(ref.load_fixture(name)[0])
        run = subprocess.run([_build_host(True), str(tmp_path / "s.jpg"), str(tmp_path / "o.bin")], capture_output=True, text=True)
        assert run.returncode == 0, name + run.stderr[-2000:]


# ---- the C++ adapter --------------------------------------------------------------------------------------------------------
def test_adapter_compiles_against_a_stand_in_decoder_device(tmp_path):
    """host/mjpeg-hip.{h,cpp} against a DecoderDevice declared here (the reference's interface, include/decoder/decoder.h: one
    pure virtual decode(char*, int, int, int, char*)); no reference tree, no OpenCV.  Without a device the constructor reports
    -3 and decode returns it."""
    inc = tmp_path / "decoder"
    inc.mkdir()
    (inc / "decoder.h").write_text("class DecoderDevice {\npublic:\n    explicit DecoderDevice();\n"
                                   "    virtual int decode(char* in, int len, int width, int height, char* out) = 0;\n};\n")
    (tmp_path / "main.cpp").write_text(r"""
#include <cstdio>
#include <decoder/mjpeg-hip.h>
DecoderDevice::DecoderDevice() {}
int main() {
    HIPMJPEGDecoder hip(64, 48);
    DecoderDevice* d = &hip;                     // what main.cpp:126 holds
    char in[4] = {(char)0xff, (char)0xd8, (char)0xff, (char)0xd9}, out[64 * 48 * 3];
    printf("status=%d decode=%d\n", hip.status(), d->decode(in, 4, 64, 48, out));
    return 0;
}
""")
    shutil.copy(os.path.join(HOST, "mjpeg-hip.h"), inc / "mjpeg-hip.h")
    libdir = os.path.join(ROOT, "rt-depth-map_amd", "lib")
    exe = str(tmp_path / "adapter")
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-I", str(tmp_path), "-I", HOST,
                           "-I", os.path.join(ROOT, "include"), str(tmp_path / "main.cpp"), os.path.join(HOST, "mjpeg-hip.cpp"),
                           "-L", libdir, "-lrtdm_host", "-lrtdm_hip", "-Wl,-rpath," + libdir, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    import torch
    if not torch.cuda.is_available():
        assert "status=-3 decode=-3" in out.stdout
    else:
        assert "status=0 decode=-8" in out.stdout           # SOI + EOI: no SOS
