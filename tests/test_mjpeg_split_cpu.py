"""The split decoder of a frame without restart intervals (rtdm_mjpeg.h: mjpeg_split_pass and its helpers; DESIGN.md section
4.12) on the CPU, before it meets a GPU.  tests/mjpeg_split_host.cpp replays the workgroup of k_mjpeg_huff_split as loops; its
coefficients and status are held against those of tests/mjpeg_host.cpp, the one-lane loop, which test_mjpeg_cpu.py pins to
NumPy and Pillow.  The tolerance is zero everywhere.  The stand-alone program is also built with -fsanitize=address,undefined;
nothing is loaded into Python under a sanitizer."""
import os
import re
import subprocess

import numpy as np
import pytest

import mjpeg_hostbuild as hb
import mjpeg_ref as ref
import mjpeg_synth as synth
from conftest import ROOT, load
from mjpeg_split_cases import SATURATING_STEPS, entropy_len, plan, saturating_dc_stream, without_dri

OK, BAD_PARAM, NULL, BAD_STREAM = 0, -1, -7, -8
SIZES = (8, 9, 16, 37, 64, 256, 4096)


def build_split(sanitize):
    key = "split_san" if sanitize else "split"
    if key not in hb._BUILT:
        exe = os.path.join(hb.tmpdir(), key)
        flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
        subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-Werror", *flags, "-I", hb.CSRC,
                               os.path.join(ROOT, "tests", "mjpeg_split_host.cpp"), "-o", exe])
        hb._BUILT[key] = exe
    return hb._BUILT[key]


def split_records(path, count):
    """[(parse status, decode status, nsub, rounds, int16 coefficients)]"""
    raw, out, p = open(path, "rb").read(), [], 0
    for _ in range(count):
        head = np.frombuffer(raw[p:p + 20], np.int32)
        p += 20
        n = int(head[2]) * 64
        out.append((int(head[0]), int(head[1]), int(head[3]), int(head[4]), np.frombuffer(raw[p:p + 2 * n], np.int16)))
        p += 2 * n
    assert p == len(raw)
    return out


def run_split(stream, workdir, sizes, sanitize=False, corruptions=()):
    """-> {S: [record per corruption, or the one record of the stream itself]}; a sanitizer report fails the run"""
    src, dst = os.path.join(str(workdir), "s.jpg"), os.path.join(str(workdir), "split.bin")
    open(src, "wb").write(stream)
    args = [str(v) for c in corruptions for v in c]
    run = subprocess.run([build_split(sanitize), src, dst, ",".join(str(s) for s in sizes), *args], capture_output=True, text=True)
    assert run.returncode == 0 and not run.stderr, run.stderr[-3000:]
    per = max(1, len(corruptions))
    recs = split_records(dst, per * len(sizes))
    return {s: recs[i * per:(i + 1) * per] for i, s in enumerate(sizes)}


def one_lane(stream, workdir, corruptions=()):
    run, recs = hb.run_host(stream, workdir, corruptions=corruptions)
    assert run.returncode == 0, run.stderr[-2000:]
    return recs


def same_as_one_lane(stream, workdir, sizes, label, sanitize=False):
    (pst, dst, coef), = one_lane(stream, workdir)
    assert pst == OK
    got = run_split(stream, workdir, sizes, sanitize)
    for S in sizes:
        (p2, d2, nsub, rounds, c2), = got[S]
        assert (p2, d2) == (pst, dst), (label, S)
        assert nsub == plan(entropy_len(stream), S)[0] and rounds <= nsub, (label, S, nsub, rounds)
        assert (rounds > 0) == (nsub >= 2), (label, S)
        if dst == OK:
            assert np.array_equal(c2, coef), (label, S)
    return got


def _has_dri(name):
    return ref.parse(ref.load_fixture(name)[0], ref.std_tables()).ri > 0


WITH_DRI = [n for n in ref.FIXTURES if _has_dri(n)]
NO_DRI = [n for n in ref.FIXTURES if n not in WITH_DRI]


def test_both_kinds_of_fixture_exist():
    assert len(NO_DRI) >= 8 and len(WITH_DRI) >= 5, (NO_DRI, WITH_DRI)


@pytest.mark.parametrize("name", NO_DRI)
def test_fixture_coefficients_and_status(tmp_path, name):
    stream = ref.load_fixture(name)[0]
    same_as_one_lane(stream, tmp_path, SIZES, name)
    same_as_one_lane(stream, tmp_path, SIZES, name, sanitize=True)


@pytest.mark.parametrize("letter", "abcde")
def test_class_streams_without_dri(tmp_path, letter):
    items = without_dri(letter)
    assert len(items) >= 9
    cut = 0
    for label, s in items:
        assert ref.parse(s, ref.std_tables()).ri == 0 and synth.launch_shape(s, ref.std_tables())[0] == 1, label
        got = same_as_one_lane(s, tmp_path, SIZES, label)
        same_as_one_lane(s, tmp_path, (8, 37), label, sanitize=True)
        cut += got[8][0][2] >= 2
    assert cut >= len(items) // 2                                       # most of them are long enough for several lanes


def test_eight_byte_subsequences_make_lanes_overshoot(tmp_path):
    """At S = 8 a symbol with its extra bits can be longer than a subsequence (up to 16 + 11 bits of a DC symbol, 16 + 10 of an AC
    one) and self-synchronisation takes more than one lane's bytes: lanes exit beyond the next lane's subsequence and start at or
    past their own end.  The rounds show it: more than the two a stream needs whose lanes all guess right."""
    stream = ref.load_fixture("mjpeg_40x24_444_q100_noise")[0]
    got = same_as_one_lane(stream, tmp_path, (8, 4096), "noise")
    assert got[8][0][2] >= 64 and got[8][0][3] > 2
    assert got[4096][0][2] == 1 and got[4096][0][3] == 0


def test_ff00_pair_at_the_cut(tmp_path):
    """Streams whose blocks end in ten 1-bits hold many FF 00 pairs.  S is stepped so that cuts fall between FF and 00 (the lane
    must start one byte later) and just after 00 (the lane before it must not take the 00 for data)."""
    between = after = 0
    for label, s in without_dri("d"):
        if "stuffed_tail" not in label:
            continue
        lo, hi = ref.entropy_range(s)
        pairs = {m.start() for m in re.finditer(b"\xff\x00", s[lo:hi])}
        assert len(pairs) >= 4, label
        sizes = []
        for S in range(8, 48):
            nsub, sp = plan(hi - lo, S)
            cuts = {i * sp for i in range(1, nsub)}
            b, a = len({c - 1 for c in cuts} & pairs), len({c - 2 for c in cuts} & pairs)
            if a or b:
                sizes.append(S)
                between, after = between + b, after + a
        if sizes:
            same_as_one_lane(s, tmp_path, sizes, label)
            same_as_one_lane(s, tmp_path, sizes[:4], label, sanitize=True)
    assert between >= 8 and after >= 8, (between, after)


def test_saturating_dc_walk(tmp_path):
    stream = saturating_dc_stream()
    (pst, dst, coef), = one_lane(stream, tmp_path)
    assert (pst, dst) == (OK, OK)
    dc = coef.reshape(-1, 64)[:, 0].astype(np.int64)
    luma, cb = dc[:120], dc[120:180]
    assert luma.max() == 32767 and luma.min() == -32768 and cb.min() == -32768 and cb.max() == 32767          # the clamp acted ...
    assert not np.array_equal(luma, np.cumsum(SATURATING_STEPS))                                                        # ... and mattered
    got = same_as_one_lane(stream, tmp_path, (8, 9, 16, 37, 64), "saturating")
    same_as_one_lane(stream, tmp_path, (8, 37), "saturating", sanitize=True)
    assert got[8][0][2] >= 32


def test_clamp_maps_compose_exactly(tmp_path):
    """mjpeg_clamp_then against the walk it stands for: random runs of differences, cut at random places, composed piece by piece
    (also far beyond the +-65536 at which a map's offset is pinned) and applied to every start value that can occur."""
    src = os.path.join(str(tmp_path), "clamp.cpp")
    open(src, "w").write(r"""
#include <cstdio>
#include <cstdlib>
#include "rtdm_mjpeg.h"
using namespace rtdm;
int main() {
    unsigned seed = 12345;
    for (int trial = 0; trial < 400; ++trial) {
        const int n = 1 + rand_r(&seed) % 200, big = trial % 3;
        int diff[200];
        for (int i = 0; i < n; ++i) diff[i] = (big == 0 ? rand_r(&seed) % 65535 - 32767 : (big == 1 ? rand_r(&seed) % 4095 - 2047 : (i % 50 < 40 ? 32767 : -32767)));
        MjpegClamp total = mjpeg_clamp_id(), piece = mjpeg_clamp_id();
        for (int i = 0; i < n; ++i) {
            MjpegClamp g = mjpeg_clamp_id();
            g.a = diff[i];
            piece = mjpeg_clamp_then(piece, g);
            if (rand_r(&seed) % 7 == 0 || i == n - 1) { total = mjpeg_clamp_then(total, piece); piece = mjpeg_clamp_id(); }
        }
        if (total.a < -65536 || total.a > 65536 || total.l < -32768 || total.h > 32767 || total.l > total.h) return 3;
        for (int x = -32768; x <= 32767; x += (x > -32700 && x < 32700 ? 97 : 1)) {
            int want = x;
            for (int i = 0; i < n; ++i) { want += diff[i]; want = want < -32768 ? -32768 : (want > 32767 ? 32767 : want); }
            if (mjpeg_clamp_apply(total, x) != want) { printf("trial %d x %d\n", trial, x); return 1; }
        }
    }
    return 0;
}
""")
    exe = os.path.join(str(tmp_path), "clamp")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", hb.CSRC, src, "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and not run.stderr, run.stdout + run.stderr[-2000:]


def test_single_byte_damage(tmp_path):
    """The eight stored corruptions of the 33x17 stream and the 64 seeded ones, through the plain and the sanitized build: the
    status of the one-lane loop each time, its coefficients wherever that status is 0, never more rounds than subsequences, and no
    report from either sanitizer (a report fails run_split)."""
    stream, _, z = ref.load_fixture("mjpeg_33x17_422_q90_corrupt")
    stored = list(zip(z["corrupt_pos"].tolist(), z["corrupt_val"].tolist()))
    todo = stored + [c for c in ref.corruptions(stream, ref.CORRUPT_SEED, ref.CORRUPT_COUNT) if c not in stored]
    assert len(stored) == 8 and len(todo) == 64
    todo += ref.corruptions(stream, ref.CORRUPT_SEED + 1, 8)
    want = one_lane(stream, tmp_path, corruptions=todo)
    assert {d for _, d, _ in want} == {OK, BAD_STREAM}
    sizes = (8, 9, 16, 37, 64)
    for sanitize in (False, True):
        got = run_split(stream, tmp_path, sizes, sanitize, corruptions=todo)
        for S in sizes:
            for c, (pst, dst, coef), (p2, d2, nsub, rounds, c2) in zip(todo, want, got[S]):
                assert (p2, d2) == (pst, dst), (c, S)
                assert nsub == plan(entropy_len(stream), S)[0] and 1 <= rounds <= nsub, (c, S, nsub, rounds)
                if dst == OK:
                    assert np.array_equal(c2, coef), (c, S)


@pytest.mark.parametrize("name", WITH_DRI)
def test_streams_with_dri_keep_the_one_lane_records(tmp_path, name):
    stream = ref.load_fixture(name)[0]
    (pst, dst, coef), = one_lane(stream, tmp_path)
    for S, ((p2, d2, nsub, rounds, c2),) in run_split(stream, tmp_path, (8, 64), sanitize=True).items():
        assert (p2, d2, nsub, rounds) == (pst, dst, 0, 0), (name, S)
        assert np.array_equal(c2, coef)


def test_plan_and_lane_counts(tmp_path):
    """mjpeg_split_plan and mjpeg_split_lanes at their edges, printed by a program built against the header"""
    src = os.path.join(str(tmp_path), "plan.cpp")
    open(src, "w").write(r"""
#include <cstdio>
#include <cstdlib>
#include "rtdm_mjpeg.h"
int main(int argc, char** argv) {
    for (int i = 1; i + 1 < argc; i += 2) {
        uint32_t sp = 0;
        const uint32_t n = rtdm::mjpeg_split_plan((uint32_t)atol(argv[i]), (uint32_t)atol(argv[i + 1]), &sp);
        printf("%u %u %u\n", n, sp, rtdm::mjpeg_split_lanes(n));
    }
    return 0;
}
""")
    exe = os.path.join(str(tmp_path), "plan")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-Werror", "-I", hb.CSRC, src, "-o", exe])
    cases = {(100, 0): (0, 0, 64), (0, 8): (0, 0, 64), (8, 8): (1, 8, 64), (9, 8): (2, 8, 64), (512, 8): (64, 8, 64),
             (513, 8): (65, 8, 128), (8192, 8): (1024, 8, 1024), (8193, 8): (911, 9, 1024), (200000, 64): (1021, 196, 1024),
             (1 << 30, 65536): (1024, 1 << 20, 1024), (2049, 8): (257, 8, 512), (4097, 8): (513, 8, 1024)}
    args = [str(v) for k in cases for v in k]
    out = subprocess.check_output([exe, *args], text=True).split("\n")
    for (k, want), line in zip(cases.items(), out):
        assert tuple(int(v) for v in line.split()) == want, (k, line)
        if want[0]:
            assert want == plan(*k) + (want[2],) and want[0] <= 1024


def test_exports_and_argument_checks():
    B = load("binding")
    L = B.lib()
    assert L.rtdm_abi_version() == 3
    text = open(os.path.join(ROOT, "include", "rtdm.h")).read()
    for n in ("rtdm_mjpeg_set_split", "rtdm_mjpeg_get_split", "rtdm_mjpeg_get_split_stats"):
        assert n in B.EXPORTS and re.search(r"\b%s\s*\(" % n, text) and hasattr(L, n), n
    # the value is judged before the handle, so that this needs no device: a value that is refused is BAD_PARAM whatever the
    # handle, a value that is accepted gets as far as the missing handle
    for v in (1, 2, 7, 65537, -2, 1 << 20):
        assert L.rtdm_mjpeg_set_split(None, v) == BAD_PARAM, v
    for v in (0, -1, 8, 256, 65536):
        assert L.rtdm_mjpeg_set_split(None, v) == NULL, v
    import ctypes as C
    v, a, b = C.c_int(), C.c_long(), C.c_long()
    assert L.rtdm_mjpeg_get_split(None, C.byref(v)) == NULL
    assert L.rtdm_mjpeg_get_split_stats(None, C.byref(a), C.byref(b), C.byref(v)) == NULL
