"""Host builds of the MJPEG decoder's plain C++ (rt-depth-map_amd/csrc/rtdm_mjpeg.h) for the CPU tests: tests/mjpeg_host.cpp
compiled with g++, plainly and with -fsanitize=address,undefined, and a tiny program that prints the built-in Huffman tables.
Each is built once per test run into a temporary directory that is removed when the interpreter exits."""
import atexit
import os
import shutil
import subprocess
import tempfile

import numpy as np

from conftest import ROOT

CSRC = os.path.join(ROOT, "rt-depth-map_amd", "csrc")

_DUMP = r"""
#include <cstdio>
#include "rtdm_mjpeg.h"
int main() {
    for (int id = 0; id < 2; ++id) for (int cls = 0; cls < 2; ++cls) {
        unsigned char bits[16], vals[256];
        if (!rtdm::mjpeg_std_table(cls, id, bits, vals)) return 1;
        int n = 0;
        for (int i = 0; i < 16; ++i) n += bits[i];
        fputc(cls << 4 | id, stdout); fwrite(bits, 1, 16, stdout); fwrite(vals, 1, n, stdout);
    }
    return 0;
}
"""
_BUILT = {}


def tmpdir():
    if "dir" not in _BUILT:
        _BUILT["dir"] = tempfile.mkdtemp(prefix="mjpeg_host_")
        atexit.register(shutil.rmtree, _BUILT["dir"], ignore_errors=True)
    return _BUILT["dir"]


def build_dump():
    if "dump" not in _BUILT:
        src = os.path.join(tmpdir(), "dump.cpp")
        open(src, "w").write(_DUMP)
        exe = os.path.join(tmpdir(), "dump")
        subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-Werror", "-I", CSRC, src, "-o", exe])
        _BUILT["dump"] = exe
    return _BUILT["dump"]


def build_host(sanitize):
    key = "host_san" if sanitize else "host"
    if key not in _BUILT:
        exe = os.path.join(tmpdir(), key)
        flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
        subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-Werror", *flags, "-I", CSRC,
                               os.path.join(ROOT, "tests", "mjpeg_host.cpp"), "-o", exe])
        _BUILT[key] = exe
    return _BUILT[key]


def records(path, count):
    """the records mjpeg_host wrote: [(parse status, decode status, int16 coefficients)]"""
    raw, out, p = open(path, "rb").read(), [], 0
    for _ in range(count):
        head = np.frombuffer(raw[p:p + 12], np.int32)
        p += 12
        n = int(head[2]) * 64
        out.append((int(head[0]), int(head[1]), np.frombuffer(raw[p:p + 2 * n], np.int16)))
        p += 2 * n
    assert p == len(raw)
    return out


def run_host(stream, workdir, sanitize=False, corruptions=()):
    """mjpeg_host on one stream (or on its copies with one byte changed each) -> (the process, its records)"""
    src, dst = os.path.join(str(workdir), "s.jpg"), os.path.join(str(workdir), "o.bin")
    open(src, "wb").write(stream)
    args = [str(v) for c in corruptions for v in c]
    run = subprocess.run([build_host(sanitize), src, dst, *args], capture_output=True, text=True)
    return run, (records(dst, max(1, len(corruptions))) if run.returncode == 0 else None)
