"""What plan_lrcheck and plan_speckle (rt-depth-map_amd/csrc/k_rows.hip) plan for the left-right check and the speckle filter,
through the stand-alone program tests/rows_plan_host.cpp: built with hipcc (host code only) into a temporary directory and
linked against librtdm_hip.so, which loads without a device.  The rows are the route table of DESIGN.md ("K3 / K4: routes"),
kept in tests/rows_cases.py; the environment hooks of a row go to the child process that plans it.  The cases of
tests/lr_cases.py (any minDisparity, speckleRange and ROI1) are pinned to their kernel form through the program's lr mode."""
import os
import re
import subprocess

import pytest

import lr_cases as LC
import rows_cases as RC
from conftest import PKG, ROOT

HOOKS = ("RTDM_LR_PAIRS", "RTDM_LR_PACKED", "RTDM_MERGE_REC_FUSED")
LR = re.compile(r"lr: form=(\w+) threads=(\d+) gy=(\d+) gz=(\d+) lds=(\d+) heads=(\w+) block_rows=(\d+) ")
SPK = re.compile(r"spk: init_lds=(\d+) heads=(\w+) rec_own=(\d+) rec_fused=(\d+) rec_rows=(\d+) rec_blk=(\d+) merge=(\S+) gx=(\d+) first=(\d+) "
                 r"npairs=(\d+) ystep=(\d+) y_hi=(\d+) rows_gx=(\d+)$")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("rows_plan") / "rows_plan_host")
    lib = os.path.join(ROOT, PKG, "lib")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, PKG, "csrc"),
                           os.path.join(ROOT, "tests", "rows_plan_host.cpp"), "-L" + lib, "-lrtdm_hip", "-Wl,-rpath," + lib, "-o", out])
    return out


def run(exe, args, env=None):
    e = {k: v for k, v in os.environ.items() if k not in HOOKS}
    e.update(env or {})
    p = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, env=e)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr
    return p.stdout.splitlines()


def parse(line):
    """-> (lr, spk): lr = (form, threads, gy, gz, lds, heads, block_rows) or None, spk = a dict or None"""
    lr = spk = None
    m = LR.search(line)
    if m:
        g = m.groups()
        lr = (g[0],) + tuple(int(v) for v in g[1:5]) + (g[5], int(g[6]))
    else:
        assert "lr: - " in line or line.startswith("sgm "), line
    m = SPK.search(line)
    if m:
        names = ("init_lds", "heads", "rec_own", "rec_fused", "rec_rows", "rec_blk", "merge", "gx", "first", "npairs", "ystep", "y_hi", "rows_gx")
        spk = {k: (v if k in ("heads", "merge") else int(v)) for k, v in zip(names, m.groups())}
    else:
        assert line.endswith("spk: -"), line
    return lr, spk


def check_spk(got, want, W, H, n, heads, nrows, what):
    init, (rec_where, rec_blocks), merge, gx, first, npairs, ystep = want
    assert got["init_lds"] == (6 * W if init else 0), what
    assert got["heads"] == heads, what
    assert (got["rec_own"], got["rec_fused"]) == (rec_blocks if rec_where == "own" else 0, rec_blocks if rec_where == "fused" else 0), what
    if rec_where:                               # the records of the pairs inside blocks of four of the checked rows
        assert (got["rec_rows"], got["rec_blk"]) == (nrows, 4), what
    assert (got["merge"], got["gx"], got["first"], got["npairs"], got["ystep"]) == (merge, gx, first, npairs, ystep), what
    assert got["rows_gx"] == (n * H + 15) // 16, what


@pytest.mark.parametrize("r", RC.BM_ROWS, ids=lambda r: "row" + r["no"])
def test_block_matcher_row(exe, r):
    line, = run(exe, ["bm", r["W"], r["H"], r["D"], r["w"], r["cap"], r["n"], r["maxdiff"], r["window"], r["aligned"]], r["env"])
    lr, spk = parse(line)
    what = (r["no"], line)
    if r["lr"] is None:
        assert lr is None, what
    else:
        form, threads, gy, lds, heads, block_rows = r["lr"]
        assert lr == (form, threads, gy, r["n"], lds, heads, block_rows), what
    if r["spk"] is None:
        assert spk is None, what
    else:
        heads = r["lr"][4] if r["lr"] else "PIXEL"           # k_spk_init writes per-pixel heads
        check_spk(spk, r["spk"], r["W"], r["H"], r["n"], heads, r["H"] - (r["w"] - 1), what)
        assert spk["y_hi"] == (r["H"] if r["lr"] is None else r["H"] - r["w"] // 2), what


@pytest.mark.parametrize("no,W,H,n,want", RC.SGM_ROWS, ids=lambda v: "row" + v if isinstance(v, str) else None)
def test_semi_global_hand_off(exe, no, W, H, n, want):
    line, = run(exe, ["sgm", W, H, n])
    lr, spk = parse(line)
    assert lr is None
    check_spk(spk, want, W, H, n, "PIXEL", H, (no, line))


def test_hooks_default_to_the_unhooked_plan(exe):
    # RTDM_LR_PAIRS=0, RTDM_LR_PACKED=1 and RTDM_MERGE_REC_FUSED=1 are the defaults
    rows = [r for r in RC.BM_ROWS if not r["env"]]
    args = ["bm"] + [v for r in rows for v in (r["W"], r["H"], r["D"], r["w"], r["cap"], r["n"], r["maxdiff"], r["window"], r["aligned"])]
    assert run(exe, args) == run(exe, args, {"RTDM_LR_PAIRS": "0", "RTDM_LR_PACKED": "1", "RTDM_MERGE_REC_FUSED": "1"})


def test_sweep_over_every_width(exe):
    # every W in 16..4096 that is a multiple of 8, n in {1, 16, 1024}, H in {w + 1, w + 3, 720} at D = 16, w = 9, cap = 31:
    # whatever is planned fits the device and leaves no row pair outside the checked rows
    lines = run(exe, ["sweep", 16, 9, 31])
    assert len(lines) == 511 * 3 * 3
    forms, merges = set(), set()
    for line in lines:
        lr, spk = parse(line)
        form, threads, gy, gz, lds, heads, block_rows = lr
        assert lds < 65536 and threads <= 512 and threads % 64 == 0 and gy >= 1, line
        assert block_rows in (1, 4) and heads == "CHUNK", line
        assert spk["first"] + (spk["npairs"] - 1) * spk["ystep"] + 1 < spk["y_hi"], line
        assert (spk["merge"] == "none") == (spk["npairs"] == 0), line
        forms.add(form); merges.add(spk["merge"])
    assert forms == {"vec_half2", "packed", "vec_wave"}
    # (strips of two pairs need a packed check and a middling launch: row 4 of the table)
    assert merges == {"none", "strip<1,chunk>", "strip<4,chunk>", "strip<1,chunk,REC>"}


@pytest.mark.parametrize("r", RC.gpu_rows(), ids=lambda r: "row" + r["no"])
def test_frames_of_the_gpu_rows_are_live(oracle, synth, r):
    # what tests/test_gpu_rows_routes.py asserts before it looks at the device, here without one: on every compared frame the
    # left-right check and the speckle filter each remove at least 5 pixels of the oracle's map and at least 100 survive
    n = r["n"]
    for f in RC.frames(r):
        L, R = synth.make_pair(synth.STREAM_SEED + RC.SEED_BASE + r["D"] + r["w"] + f, r["W"], r["H"], r["D"])
        _, lr, spk, alive = RC.liveness(oracle, r, L, R)
        print(RC.assert_live(r, f, lr, spk, alive))
    assert n == 1 or RC.frames(r) == (0, n - 1)


# ---- the cases of tests/lr_cases.py: any minDisparity, speckleRange and ROI1 (the program's lr mode) ---------------------------
LR_STATE = re.compile(r"lr: form=(\w+) init=(\d) threads=(\d+) gy=(\d+) gz=(\d+) lds=(\d+) heads=(\w+) block_rows=(\d+) rect=(-?\d+),(-?\d+),(-?\d+),(-?\d+)$")


def lr_args(c):
    return [c["W"], c["H"], c["D"], c["w"], c["cap"], c["n"], c["M"], c["window"], c["range"], c["minD"]] + list(c["roi"] or (0, 0, 0, 0))


@pytest.fixture(scope="module")
def lr_lines(exe):
    lines = run(exe, ["lr"] + [v for c in LC.CASES for v in lr_args(c)])
    assert len(lines) == len(LC.CASES)
    return {c["id"]: line for c, line in zip(LC.CASES, lines)}


@pytest.mark.parametrize("c", LC.CASES, ids=lambda c: c["id"])
def test_left_right_state_case_is_planned_on_its_form(lr_lines, oracle, c):
    line = lr_lines[c["id"]]
    m = LR_STATE.search(line)
    assert m, line
    form, init, threads, gy, gz, lds, heads, block_rows = m.group(1), int(m.group(2)), int(m.group(3)), int(m.group(4)), int(m.group(5)), \
        int(m.group(6)), m.group(7), int(m.group(8))
    assert (form, bool(init)) == (c["form"], c["init"]), line
    assert gz == c["n"] and lds < 65536 and threads <= 512 and threads % 64 == 0, line
    assert heads == ("NONE" if not init else "PIXEL" if form == "scalar_i32" else "CHUNK") and block_rows == (4 if form == "vec_half2" else 1), line
    # the program's geometry is make_geom's: the valid rectangle is the oracle's
    assert tuple(int(v) for v in m.groups()[8:]) == oracle.valid_rect(c["W"], c["H"], **LC.oracle_kw(c)), line


def test_either_side_of_every_reachable_bound_of_the_packed_form(exe):
    """two_ok_for_pk (k_rows.hip), one bound at a time around a shape that is packed: 2 cap w w < 32768, disp12MaxDiff <= 512,
    speckleRange <= 4096, minDisparity >= -1024, minDisparity + numDisparities <= 1024.  (W + 2 < 16384 and the 64 KB of LDS lie
    beyond the widest frame a handle accepts, 4096 columns: 24.6 KB.)"""
    def form(W=1208, H=11, D=64, w=9, cap=31, M=1, window=2, rng=32, minD=0):
        line, = run(exe, ["lr", W, H, D, w, cap, 1, M, window, rng, minD, 0, 0, 0, 0])
        return LR_STATE.search(line).group(1)
    assert form() == "packed"
    assert (form(w=17, cap=56, H=19), form(w=17, cap=57, H=19)) == ("packed", "vec_half") and 2 * 56 * 17 * 17 < 32768 <= 2 * 57 * 17 * 17
    assert (form(w=21, cap=37, H=23), form(w=21, cap=38, H=23)) == ("packed", "vec_half") and 2 * 37 * 21 * 21 < 32768 <= 2 * 38 * 21 * 21
    assert (form(M=512), form(M=513)) == ("packed", "vec_half")
    assert (form(rng=4096), form(rng=4097)) == ("packed", "vec_half")
    assert (form(rng=4097, window=0), form(rng=-1)) == ("packed", "packed")          # the filter is off: its range is not read
    assert (form(minD=-1024), form(minD=-1025)) == ("packed", "vec_half")
    assert (form(W=2040, minD=960), form(W=2040, minD=961)) == ("packed", "vec_half")
    assert form(W=4096, D=16, w=5, H=7, minD=0) == "vec_wave"                        # past eight half-waves the packed form is not planned
