"""rtdm::copy_rows (rt-depth-map_amd/csrc/rtdm_rows.h), the one host row copy of the C ABI layer: tests/rows_host.cpp sweeps it over
rows {0, 1, 2, 5} x row_bytes {0, 1, 7, 16} x destination and source pitches {row_bytes, row_bytes + 3, 32} x both RowPad modes on
heap buffers that end at the last row's last byte.  Compiled with plain g++ -std=c++11 (the header needs no HIP), once plainly
and once with -fsanitize=address,undefined, and run as a child process; both builds print the same line."""
import os
import subprocess

import pytest

from conftest import ROOT

CASES = 4 * 4 * 3 * 3 * 2


@pytest.fixture(scope="module")
def build(tmp_path_factory):
    out = tmp_path_factory.mktemp("rows_host")

    def make(sanitize):
        exe = str(out / ("rows_san" if sanitize else "rows"))
        flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
        subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-Werror", *flags, "-I",
                               os.path.join(ROOT, "rt-depth-map_amd", "csrc"), os.path.join(ROOT, "tests", "rows_host.cpp"), "-o", exe])
        return exe
    return make


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_copy_rows_sweep(build, sanitize):
    run = subprocess.run([build(sanitize)], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    assert run.stdout == "ok %d\n" % CASES
