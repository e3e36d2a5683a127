"""What plan_search (rt-depth-map_amd/csrc/k_search.hip) plans for the StereoBM search stage, through the stand-alone program
tests/search_plan_host.cpp: built with hipcc (host code only) into a temporary directory and linked against librtdm_hip.so,
which loads without a device.  The rows are the route table of DESIGN.md ("K2: routes"): each is the smallest frame at
which its route exists.  All rows: disp12MaxDiff = 1, no ROIs."""
import os
import re
import subprocess

import pytest

from conftest import PKG, ROOT

# (W, H, D, w, minD, cap, legacy) -> at n = 1: (tiles, lanes, border form, placement, border grid, variant)
TABLE = [
    ((300, 80, 64, 9, 0, 31, 0), ("ring", 4, "ROWS", "FUSED", "2x2", "fast_ring4_qsad")),          # 72 rows / 56 per wave
    ((560, 90, 256, 15, 0, 15, 0), ("ring", 16, "DISP", "FUSED", "4x5", "fast_ring16_qsad")),      # D = 256: no fused ROWS; two waves
    ((250, 66, 32, 9, 0, 63, 0), ("ring", 2, "DISP", "FUSED", "2x4", "fast_ring_qsad")),           # 64 w 2 cap > 65535; three waves
    ((300, 80, 64, 9, 0, 63, 0), ("ring", 4, "DISP", "AFTER", "2x5", "fast_ring4_qsad")),          # four waves fuse no DISP
    ((300, 80, 80, 9, 0, 31, 0), ("fast", 0, "DISP", "FUSED", "2x5", "fast_qsad")),
    ((300, 80, 64, 17, 0, 31, 0), ("fast", 0, "DISP", "FUSED", "4x4", "fast_qsad")),               # 5 pieces
    ((200, 50, 64, 23, 0, 30, 0), ("fast", 0, "GENERIC", "AFTER", "0x0", "fast_qsad")),            # 6 pieces; no border form above w = 21
    ((300, 80, 64, 9, -7, 31, 1), ("ring", 4, "DISP+LEGACY", "AFTER", "2x5", "fast_ring4_qsad")),
    ((300, 90, 64, 25, 0, 31, 0), ("generic", 0, "NONE", "AFTER", "0x0", "generic_u16")),
    ((400, 80, 272, 9, 0, 31, 0), ("generic", 0, "NONE", "AFTER", "0x0", "generic_dslice_u16")),
    ((1280, 720, 64, 9, 0, 31, 0), ("ring", 4, "ROWS", "FUSED", "2x13", "fast_ring4_qsad")),
    ((1280, 720, 192, 13, 0, 31, 0), ("ring", 8, "ROWS", "FUSED", "3x14", "fast_ring8_qsad")),
    ((80, 60, 64, 9, 0, 31, 0), ("ring", 4, "ROWS", "FUSED", "2x1", "fast_ring4_qsad")),
]
# the border columns of some rows
RANGES = {(200, 50, 64, 23, 0, 30, 0): ("[0,11)", "[126,137)"), (1280, 720, 64, 9, 0, 31, 0): ("[0,4)", "[1213,1217)")}
# n = 16: every border launch of its own moves to the side stream, as ROWS where that form covers the configuration
ROWS_AT_16 = {(300, 80, 64, 9, 0, 31, 0): "2x2", (560, 90, 256, 15, 0, 15, 0): "4x2", (1280, 720, 64, 9, 0, 31, 0): "2x13",
              (1280, 720, 192, 13, 0, 31, 0): "3x14", (80, 60, 64, 9, 0, 31, 0): "2x1"}

LINE = re.compile(r"tiles=(\w+) lanes=(\d+) interior=(\S+) border=(\S+) place=(\w+) left=(\S+) right=(\S+) grid=(\S+) variant=(\w+)$")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("search_plan") / "search_plan_host")
    lib = os.path.join(ROOT, PKG, "lib")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, PKG, "csrc"),
                           os.path.join(ROOT, "tests", "search_plan_host.cpp"), "-L" + lib, "-lrtdm_hip", "-Wl,-rpath," + lib, "-o", out])
    return out


def plans(exe, n, contiguous=1, env=None):
    """-> {row: dict(tiles, lanes, interior, border, place, left, right, grid, variant)} in a child process"""
    args = [str(v) for row, _ in TABLE for v in row]
    e = dict(os.environ)
    e.pop("RTDM_BORDER2", None)
    e.update(env or {})
    run = subprocess.run([exe, str(n), str(contiguous)] + args, capture_output=True, text=True, env=e)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = run.stdout.splitlines()
    assert len(lines) == len(TABLE)
    out = {}
    for (row, _), line in zip(TABLE, lines):
        m = LINE.search(line)
        assert m, line
        out[row] = dict(zip(("tiles", "lanes", "interior", "border", "place", "left", "right", "grid", "variant"), m.groups()))
        out[row]["lanes"] = int(out[row]["lanes"])
    return out


def key(p):
    return (p["tiles"], p["lanes"], p["border"], p["place"], p["grid"], p["variant"])


def test_routes_of_a_single_frame(exe):
    got = plans(exe, 1)
    for row, want in TABLE:
        assert key(got[row]) == want, (row, got[row])
    for row, (left, right) in RANGES.items():
        assert (got[row]["left"], got[row]["right"]) == (left, right), (row, got[row])
    g = got[(300, 90, 64, 25, 0, 31, 0)]
    assert g["interior"] == "[0,237)"                     # generic tiles: every searched column


def test_routes_of_a_batch_of_16(exe):
    one, got = plans(exe, 1), plans(exe, 16)
    for row, (tiles, lanes, form, place, grid, variant) in TABLE:
        p = got[row]
        assert (p["tiles"], p["lanes"], p["variant"]) == (tiles, lanes, variant), (row, p)
        assert (p["interior"], p["left"], p["right"]) == (one[row]["interior"], one[row]["left"], one[row]["right"]), (row, p)
        if form in ("NONE", "GENERIC"):                   # the generic ranges stay behind the tiles at every n
            assert (p["border"], p["place"], p["grid"]) == (form, "AFTER", "0x0"), (row, p)
        elif row in ROWS_AT_16:
            assert (p["border"], p["place"], p["grid"]) == ("ROWS", "SIDE", ROWS_AT_16[row]), (row, p)
        else:                                             # what ROWS does not cover: DISP, with its n = 1 flag
            assert (p["border"], p["place"]) == (form, "SIDE"), (row, p)


@pytest.mark.parametrize("n", [1, 16])
def test_border2_hook_plans_disp_wherever_rows_would_run(exe, n):
    on, off = plans(exe, n), plans(exe, n, env={"RTDM_BORDER2": "0"})
    nrows = 0
    for row, _ in TABLE:
        a, b = on[row], off[row]
        if a["border"] != "ROWS":
            assert a == b, (row, a, b)
            continue
        nrows += 1
        assert b["border"] == "DISP", (row, b)
        for f in ("tiles", "lanes", "interior", "left", "right", "variant"):
            assert a[f] == b[f], (row, f, a, b)
        if n == 16:
            assert b["place"] == "SIDE"
        else:
            # the four-wave ring forms carry no DISP workgroups: a launch of its own behind the tiles
            assert b["place"] == ("AFTER" if (row[2], row[3]) == (64, 9) else "FUSED"), (row, b)
    assert nrows == (5 if n == 16 else 4)


def test_planes_that_are_not_one_allocation_plan_the_fast_kernel(exe):
    on, off = plans(exe, 1), plans(exe, 1, contiguous=0)
    nring = 0
    for row, _ in TABLE:
        a, b = on[row], off[row]
        if a["tiles"] != "ring":
            assert a == b, (row, a, b)
            continue
        nring += 1
        assert (b["tiles"], b["lanes"], b["variant"]) == ("fast", 0, "fast_qsad"), (row, b)
        assert (b["interior"], b["left"], b["right"]) == (a["interior"], a["left"], a["right"]), (row, b)
        # k_search_fast carries DISP only, and not the 3.x clamp
        assert (b["border"], b["place"]) == (("DISP+LEGACY", "AFTER") if row[6] else ("DISP", "FUSED")), (row, b)
    assert nring == 8
