"""The shapes tests/test_gpu_ring_prefetch.py runs, pinned: how ring_strips_model cuts each (W, H, n) into row strips.

The paired ring search k_search_ring<64, 9, 4> reads row t + 1 from LDS at the top of step t (RingCfg::PREFETCH), across the
boundaries of row groups (four steps) and of the trips of the unrolled row loop (TRIP = 20 steps).  What can go wrong is the
bookkeeping where a strip ends, so the GPU shapes are chosen by STEPS PER STRIP = output rows of the strip + 8: 20, 21, 24, 25,
28, 40, 41, 44, 60 and 61 -- the exits behind each group position of a trip, in the first, second and third trip.  The strip
model decides how a frame is cut; this file asks the library (tests/search_plan_host.cpp `strips`) and pins the answer.

Both instantiations walk every one of the ten lengths: n = 1 (border workgroups in the grid) and n = 16 (tile-only).  A frame is
one strip (H = steps) only up to 24 steps: while the grid fits one scheduling round of the chip's 768 workgroup slots the model
cuts strips of at most 16 output rows.  Longer strips come where tiles x strips x n would need a second round, which costs more
than longer strips do: frames of several hundred rows at n = 16, and at n = 1 frames as wide as the headline's (1280 columns,
19 tiles), 649 to 2089 rows high -- a single 1280 x 720 frame itself is cut into 40 strips of 18 rows, 26 steps.  Those frames
are many strips, the first inside the frame's top, the others starting inside the frame.  Batches of 2048 small frames give
every length as a single strip too (the tile-only instantiation again)."""
import os
import re
import subprocess

import pytest

from conftest import PKG, ROOT

D, WS, CAP = 64, 9, 31
TRIP, RPG = 20, 4
STEPS = (20, 21, 24, 25, 28, 40, 41, 44, 60, 61)

# (W, H, n, strips, output rows per strip)
ONE_STRIP = tuple((W, H, n, 1, H - (WS - 1)) for n in (1, 16) for W in (128, 200) for H in (20, 21, 24)) + \
            tuple((W, H, 2048, 1, H - (WS - 1)) for W in (128, 200) for H in STEPS)
# strips that start inside the frame; the last one runs into the clamped rows below H - 1 (its read-ahead and staging do)
MULTI_STRIP = ((128, 40, 1, 2, 16), (200, 40, 1, 2, 16), (128, 40, 16, 2, 16), (200, 40, 16, 2, 16),
               (200, 100, 16, 6, 16),          # the 16-frame batch: five strips of 24 steps and one of 20
               (128, 107, 1024, 3, 33))        # three strips of 41 steps: two trips and a group
# the strips above 24 steps in batches of 16 frames, at both widths, and in single frames (as wide as the headline's, and the
# headline frame itself): the model lengthens the strips where the grid would otherwise need a second scheduling round
LONG_STEPS = (25, 28, 40, 41, 44, 60, 61)
LONG_N16 = ((200, 265, 16, 16, 17), (200, 313, 16, 16, 20), (200, 505, 16, 16, 32), (200, 521, 16, 16, 33), (200, 569, 16, 16, 36),
            (200, 825, 16, 16, 52), (200, 841, 16, 16, 53),
            (128, 777, 16, 46, 17), (128, 921, 16, 46, 20), (128, 1497, 16, 47, 32), (128, 1545, 16, 47, 33), (128, 1689, 16, 47, 36),
            (128, 2457, 16, 48, 52), (128, 2505, 16, 48, 53))
LONG_N1 = ((1280, 649, 1, 38, 17), (1280, 720, 1, 40, 18), (1280, 769, 1, 39, 20), (1280, 1249, 1, 39, 32), (1280, 1289, 1, 39, 33),
           (1280, 1409, 1, 39, 36), (1280, 2049, 1, 40, 52), (1280, 2089, 1, 40, 53))
MULTI_STRIP = MULTI_STRIP + LONG_N16 + LONG_N1
CASES = ONE_STRIP + MULTI_STRIP

LINE = re.compile(r"n=(\d+): lanes=(\d+) strips=(\d+) rows_per_strip=(\d+) rebase_rows=(\d+)$")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("ring_prefetch") / "search_plan_host")
    lib = os.path.join(ROOT, PKG, "lib")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, PKG, "csrc"),
                           os.path.join(ROOT, "tests", "search_plan_host.cpp"), "-L" + lib, "-lrtdm_hip", "-Wl,-rpath," + lib, "-o", out])
    return out


def strips_of(exe, n, shapes):
    """-> [(lanes, strips, rows per strip)] for the (W, H) of `shapes`, all in a batch of n"""
    args = [str(v) for W, H in shapes for v in (W, H, D, WS, 0, CAP, 0)]
    run = subprocess.run([exe, "strips", str(n)] + args, capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = run.stdout.strip().split("\n")
    assert len(lines) == len(shapes), run.stdout
    out = []
    for line in lines:
        m = LINE.search(line)
        assert m and int(m.group(1)) == n, line
        out.append((int(m.group(2)), int(m.group(3)), int(m.group(4))))
    return out


def test_every_gpu_shape_is_cut_as_pinned(exe):
    for n in sorted({c[2] for c in CASES}):
        rows = [c for c in CASES if c[2] == n]
        got = strips_of(exe, n, [(c[0], c[1]) for c in rows])
        for (W, H, _, strips, rs), (lanes, gs, grs) in zip(rows, got):
            assert lanes == 4, (W, H, n, lanes)
            assert (gs, grs) == (strips, rs), "%dx%d n=%d: %d strips of %d rows, pinned %d of %d" % (W, H, n, gs, grs, strips, rs)
            assert (strips - 1) * rs < H - (WS - 1) <= strips * rs


def test_the_single_strip_shapes_cover_every_exit_of_the_row_loop():
    for W in (128, 200):
        steps = {rs + WS - 1 for w, H, n, strips, rs in ONE_STRIP if w == W}
        assert steps == set(STEPS), (W, sorted(steps))
        assert all(H == rs + WS - 1 for w, H, n, strips, rs in ONE_STRIP if w == W)       # H = steps when a frame is one strip
    # a frame of a batch of 1 or 16 is one strip only up to 24 steps (longer strips: the multi-strip shapes, below)
    for n in (1, 16):
        assert {rs + WS - 1 for W, H, m, strips, rs in ONE_STRIP if m == n} == {20, 21, 24}
    # what the lengths stand for: with groups of four, padded, the loop ends behind group 5, 10 or 15 (the last of a trip: the
    # read-ahead of the last step is never used), 6, 11 or 16 (the first of the next trip) and 7 (its second)
    groups = sorted({(s + RPG - 1) // RPG for s in STEPS})
    assert groups == [5, 6, 7, 10, 11, 15, 16]
    assert {(g - 1) % (TRIP // RPG) for g in groups} == {0, 1, 4}
    assert {(g - 1) // (TRIP // RPG) for g in groups} == {0, 1, 2, 3}
    assert {s % RPG for s in STEPS} == {0, 1}                       # whole last groups, and padded ones with three dropped rows


def test_both_instantiations_walk_every_length():
    # n = 1: the border workgroups ride in the grid; n = 16: tile-only.  Single strips up to 24 steps, strips of longer frames above
    for n in (1, 16):
        steps = {rs + WS - 1 for W, H, m, strips, rs in CASES if m == n}
        assert steps >= set(STEPS), (n, sorted(set(STEPS) - steps))
    for W in (128, 200):                                            # at n = 16 at both widths of the single-strip cases
        assert {rs + WS - 1 for w, H, n, strips, rs in LONG_N16 if w == W} == set(LONG_STEPS)
    assert {rs + WS - 1 for W, H, n, strips, rs in LONG_N1} == set(LONG_STEPS) | {26}   # (26: the headline's 1280 x 720 frame)


def test_the_multi_strip_shapes_have_strips_inside_the_frame():
    for W, H, n, strips, rs in MULTI_STRIP:
        assert strips >= 2
        last = H - (WS - 1) - (strips - 1) * rs
        assert 0 < last <= rs
    assert any(n == 16 and strips >= 2 for W, H, n, strips, rs in MULTI_STRIP)
    # strips of 41 steps cross two trip boundaries with the read-ahead in flight
    assert any(rs + WS - 1 > 2 * TRIP for W, H, n, strips, rs in MULTI_STRIP)
