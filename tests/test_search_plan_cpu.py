"""What plan_search (rt-depth-map_amd/csrc/k_search.hip) plans for the StereoBM search stage, through the stand-alone program
tests/search_plan_host.cpp: built with hipcc (host code only) into a temporary directory and linked against librtdm_hip.so,
which loads without a device.  The rows are the route table of DESIGN.md ("K2: routes"): each is the smallest frame at
which its route exists.  All rows: disp12MaxDiff = 1, no ROIs."""
import os
import re
import subprocess

import pytest

import hostile_cases
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


def plans(exe, n, contiguous=1, env=None, rows=None):
    """-> {row: dict(tiles, lanes, interior, border, place, left, right, grid, variant)} in a child process; rows: the rows of
    TABLE unless given"""
    rows = [row for row, _ in TABLE] if rows is None else list(rows)
    e = dict(os.environ)
    e.pop("RTDM_BORDER2", None)
    e.update(env or {})
    run = subprocess.run([exe, str(n), str(contiguous)] + [str(v) for row in rows for v in row], capture_output=True, text=True, env=e)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = run.stdout.splitlines()
    assert len(lines) == len(rows)
    out = {}
    for row, line in zip(rows, lines):
        m = LINE.search(line)
        assert m, line
        out[row] = dict(zip(("tiles", "lanes", "interior", "border", "place", "left", "right", "grid", "variant"), m.groups()))
        out[row]["lanes"] = int(out[row]["lanes"])
    return out


STRIPS = re.compile(r"n=(\d+): lanes=(\d+) strips=(\d+) rows_per_strip=(\d+) rebase_rows=(\d+)$")


def strips(exe, n, row):
    """-> (lanes per pixel, strips, output rows per strip, rows between two rebases) of the ring launch of a batch of n"""
    run = subprocess.run([exe, "strips", str(n)] + [str(v) for v in row], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    m = STRIPS.search(run.stdout.strip())
    assert m and int(m.group(1)) == n, run.stdout
    return tuple(int(v) for v in m.groups()[1:])


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


def test_largest_cap_of_every_route(exe):
    # hostile_cases.MAXCAP: the route of a row is the same at that cap, at n = 1 and n = 16, and (below 63) not one step up
    assert set(hostile_cases.MAXCAP) == {row for row, _ in TABLE[:10]}
    for n in (1, 16):
        base = plans(exe, n)
        top = plans(exe, n, rows=[hostile_cases.with_cap(r, c) for r, c in hostile_cases.MAXCAP.items()])
        over = plans(exe, n, rows=[hostile_cases.with_cap(r, c + 1) for r, c in hostile_cases.MAXCAP.items() if c < 63])
        same = lambda a, b: all(a[f] == b[f] for f in ("tiles", "lanes", "border", "place", "grid", "variant"))
        for r, c in hostile_cases.MAXCAP.items():
            assert same(base[r], top[hostile_cases.with_cap(r, c)]), (n, r, c, base[r], top[hostile_cases.with_cap(r, c)])
            assert c >= r[5]
        if n == 16:                                       # (at n = 1 the 256-disparity row runs DISP at every cap)
            for r, c in hostile_cases.MAXCAP.items():
                if c < 63:
                    assert not same(base[r], over[hostile_cases.with_cap(r, c + 1)]), (r, c + 1, over[hostile_cases.with_cap(r, c + 1)])


@pytest.mark.parametrize("n,row,lpp", hostile_cases.LONG_STRIPS + hostile_cases.LONG_STRIPS_64_9_4)
def test_long_strip_batches_walk_more_than_two_rebase_intervals(exe, n, row, lpp):
    # what tests/test_gpu_search_hostile.py and tests/test_gpu_ring_pair.py rest on: at these batch sizes the model cuts a frame
    # into strips that walk (output rows + w - 1) more rows than two rebase intervals, so both prefix rings of a workgroup
    # are rebased at least twice at the worst-case growth.  (One compute_device call per handle: the tuner keeps the model.)
    lanes, count, rs, rebase_rows = strips(exe, n, row)
    W, H, D, w, minD, cap = row[:6]
    assert lanes == lpp
    assert rebase_rows == hostile_cases.ring_rebase_trips(D, w, lpp, cap) * hostile_cases.ring_trip(D, w, lpp) > 0
    assert count * rs >= H - (w - 1) > (count - 1) * rs
    assert rs + w - 1 > 2 * rebase_rows, (rs, w, rebase_rows)
    assert n * H * W * 2 <= 45e6 or (D, w, lpp) == (64, 9, 4)      # device input of the new batches: about 40 MB at most


def test_border_forms_of_the_hostile_border_rows(exe):
    rows = [hostile_cases.BORDER_ROWS_ROW, hostile_cases.BORDER_DISP_ROW]
    one, many = plans(exe, 1, rows=rows), plans(exe, 16, rows=rows)
    r, d = rows
    assert (one[r]["border"], one[r]["place"], one[r]["variant"]) == ("ROWS", "FUSED", "fast_ring4_qsad"), one[r]
    assert (many[r]["border"], many[r]["place"]) == ("ROWS", "SIDE"), many[r]
    assert 64 * r[3] * 2 * r[5] <= 65535 < 64 * r[3] * 2 * (r[5] + 1)
    assert (one[d]["border"], one[d]["place"], one[d]["variant"]) == ("DISP", "FUSED", "fast_qsad"), one[d]
    assert (many[d]["border"], many[d]["place"]) == ("DISP", "SIDE"), many[d]
    assert 2 * d[5] * d[3] ** 2 <= 32766 < 2 * (d[5] + 1) * d[3] ** 2


@pytest.mark.parametrize("n,row,lpp", hostile_cases.NO_REBASE_STRIPS)
def test_forms_that_do_not_rebase_get_strips_of_the_full_allowed_length(exe, n, row, lpp):
    # every form of the ring table whose trip is longer than ring_rows_cap at cap 63, and no other
    lanes, count, rs, rebase_rows = strips(exe, n, row)
    W, H, D, w, minD, cap = row[:6]
    assert lanes == lpp and rebase_rows == 0 == hostile_cases.ring_rebase_trips(D, w, lpp, cap)
    assert count == 3 and rs == hostile_cases.ring_rows_cap(w, cap) and H - (w - 1) == 3 * rs
    assert n * H * W * 2 <= 45e6


def test_the_forms_that_do_not_rebase_are_all_listed():
    from test_gpu_fuzz import RING_TABLE
    none = {(D, w, lpp) for D, w, lpp in RING_TABLE for cap in (31, 63) if hostile_cases.ring_rebase_trips(D, w, lpp, cap) == 0}
    assert none == {(r[2], r[3], lpp) for _, r, lpp in hostile_cases.NO_REBASE_STRIPS}
    assert all(hostile_cases.ring_rebase_trips(D, w, lpp, 31) > 0 for D, w, lpp in RING_TABLE)
