"""The texture bookkeeping of the paired ring search (k_search_ring.hip: RingTexture), restated in numpy and checked against the
plain 9 x 9 sum of |v - cap|.

One wave holds 8 column pairs, four columns apart: lane (p, h) owns column 4 p + j (j = h & 1) in row k = h >> 1 of every group
of four rows.  Its copy of a left row is 11 dwords; the window of column c is the copy's bytes c + 3 .. c + 11.  Per group the
owner forms ITS row's term from the dwords p + 1 and p + 2 and one edge byte (byte 3 of dword p, or byte 0 of dword p + 3),
the four terms of a column become prefix sums (carried prefix + the terms of the rows <= k, by 0/1 weights), the prefix goes
into a ring of u16 [column][20] indexed by the row step modulo 20, and the window sum is the prefix minus the one nine rows back,
modulo 2^16.  The ring starts zeroed; the rows of a padded last group are computed and dropped."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import PKG, ROOT

WS, RPG, TRIP, PAIRS = 9, 4, 20, 8
COPY = 4 * (PAIRS + 3)                       # bytes of the wave's copy of a left row
COLS = [4 * p + j for p in range(PAIRS) for j in range(2)]


def owner_terms(copy_row, cap):
    """-> the 16 row terms [pair * 2 + j] as the owners form them: two shared dwords and one edge byte"""
    dw = np.frombuffer(copy_row.tobytes(), "<u4")
    capb = np.uint32(cap * 0x01010101)

    def sad_u8(a, b):
        return sum(abs(int((a >> s) & 0xff) - int((b >> s) & 0xff)) for s in (0, 8, 16, 24))
    out = []
    for p in range(PAIRS):
        shared = sad_u8(int(dw[p + 1]), int(capb)) + sad_u8(int(dw[p + 2]), int(capb))
        for j in range(2):
            edge = int(copy_row[4 * p + 12]) if j else int(dw[p] >> 24)      # (a zero-extended byte: one live byte)
            out.append(shared + abs(edge - cap))
    return np.array(out, np.uint32)


def back_index(U, k):
    """ring index of the prefix nine rows behind row k of the group at unrolled step U, as the kernel addresses it"""
    lo = U - WS
    if lo < 0 <= lo + RPG - 1:                 # the wrap falls between the group's rows: a lane-constant address of its own
        assert lo == -1
        return (k + TRIP - 1) % TRIP
    idx = (lo + TRIP) % TRIP
    assert idx + RPG - 1 < TRIP                # base + immediate: no wrap inside the group
    return idx + k


def ring_texture(copy, cap, nout):
    """copy: uint8 [rows, COPY], the rows a strip of nout output rows walks -- nout + 8 and the padding of the last group.
    -> window sums [nout, 16]"""
    nsteps = nout + WS - 1
    nstepsg = (nsteps + RPG - 1) // RPG * RPG
    assert copy.shape == (nstepsg, COPY)
    ring = np.zeros((16, TRIP), np.uint16)
    carry = np.zeros(16, np.uint32)
    w_lo = [(1, 0), (1, 1), (1, 1), (1, 1)]    # weights of rows (0, 1) for the owner of row k
    w_hi = [(0, 0), (0, 0), (1, 0), (1, 1)]    # ... of rows (2, 3)
    out = np.full((nout, 16), -1, np.int64)
    for t in range(0, nstepsg, RPG):
        U = t % TRIP
        back = np.stack([ring[:, back_index(U, k)] for k in range(RPG)]).astype(np.uint32)      # read before the group's writes
        terms = np.stack([owner_terms(copy[t + k], cap) for k in range(RPG)]).astype(np.uint16)   # u16 [k][column]
        tq = terms.astype(np.uint32)
        for k in range(RPG):
            own = carry + tq[0] * w_lo[k][0] + tq[1] * w_lo[k][1] + tq[2] * w_hi[k][0] + tq[3] * w_hi[k][1]   # (mod 2^32)
            ring[:, U + k] = (own & 0xffff).astype(np.uint16)
            y = t + k - (WS - 1)
            if 0 <= y < nout:
                out[y] = (own - back[k]) & 0xffff
        carry = carry + tq.sum(0, dtype=np.uint32)
    assert (out >= 0).all()
    return out


def plain_sums(copy, cap, nout):
    a = np.abs(copy.astype(np.int64) - cap)
    return np.array([[a[y:y + WS, c + 3:c + 3 + WS].sum() for c in COLS] for y in range(nout)])


def planes(kind, rng, rows, cap):
    if kind == "random":
        return rng.integers(0, 2 * cap + 1, (rows, COPY), dtype=np.uint8)
    if kind == "saturated":                    # every byte 0 or 2 cap: every row term is 9 cap, the most there is
        return (rng.integers(0, 2, (rows, COPY)) * 2 * cap).astype(np.uint8)
    return np.full((rows, COPY), cap, np.uint8)   # no texture at all


def check(kind, nout, cap, seed):
    rng = np.random.default_rng([seed, nout, cap])
    nstepsg = (nout + WS - 1 + RPG - 1) // RPG * RPG
    copy = planes(kind, rng, nstepsg, cap)
    copy[nout + WS - 1:] = rng.integers(0, 256, (nstepsg - (nout + WS - 1), COPY), dtype=np.uint8)   # padded rows: anything
    got, want = ring_texture(copy, cap, nout), plain_sums(copy, cap, nout)
    assert np.array_equal(got, want), "%s nout %d cap %d: first difference at %s" % (kind, nout, cap, tuple(np.argwhere(got != want)[0]))
    if kind == "saturated":
        assert (want == 81 * cap).all()


def test_owner_terms_are_the_nine_byte_row_sums():
    rng = np.random.default_rng(5)
    for cap in (1, 31, 63):
        row = rng.integers(0, 2 * cap + 1, COPY, dtype=np.uint8)
        want = [int(np.abs(row[c + 3:c + 12].astype(int) - cap).sum()) for c in COLS]
        assert owner_terms(row, cap).tolist() == want


def test_back_index_is_nine_rows_behind_in_every_group():
    for U in range(0, TRIP, RPG):
        for k in range(RPG):
            assert back_index(U, k) == (U + k - WS) % TRIP
    # nine behind is never one of the rows the group itself writes
    assert all(back_index(U, k) not in range(U, U + RPG) for U in range(0, TRIP, RPG) for k in range(RPG))


@pytest.mark.parametrize("kind", ("random", "saturated", "flat"))
def test_every_strip_length(kind):
    # all residues modulo four (padded last groups of one to three rows and none), window-filling groups only (nout = 1 .. 4
    # store from the third group on), ring indices past one (nout + 8 > 20) and two (> 40) trips
    for nout in range(1, 46):
        for cap in (31, 63):
            check(kind, nout, cap, 1)


@pytest.mark.parametrize("kind", ("random", "saturated"))
def test_prefix_wraps_16_bits(kind):
    # 148 rows of 9 x 63 each: the 16-bit prefix wraps past row 115
    nout, cap = 140, 63
    assert (nout + WS - 1) * 9 * cap > 65535
    check(kind, nout, cap, 2)


# ---- the batch tests/test_gpu_ring_texture.py wraps the prefix with ---------------------------------------------------------
WRAP_BATCH = (8192, (80, 400, 64, 9, 0, 63, 0))     # (frames, (W, H, D, w, minD, cap, legacy))
STRIPS = re.compile(r"n=(\d+): lanes=(\d+) strips=(\d+) rows_per_strip=(\d+) rebase_rows=(\d+)$")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("ring_texture") / "search_plan_host")
    lib = os.path.join(ROOT, PKG, "lib")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, PKG, "csrc"),
                           os.path.join(ROOT, "tests", "search_plan_host.cpp"), "-L" + lib, "-lrtdm_hip", "-Wl,-rpath," + lib, "-o", out])
    return out


def test_the_wrap_batch_walks_more_rows_than_the_prefix_holds(exe):
    n, row = WRAP_BATCH
    W, H, D, w, minD, cap = row[:6]
    run = subprocess.run([exe, "strips", str(n)] + [str(v) for v in row], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    m = STRIPS.search(run.stdout.strip())
    assert m and int(m.group(1)) == n, run.stdout
    lanes, count, rs, rebase_rows = (int(v) for v in m.groups()[1:])
    assert lanes == 4
    assert (count, rs) == (3, 131), run.stdout             # ring_strips_model: 392 valid rows in three strips
    assert rs + w - 1 > 65536 // (w * cap)                  # a strip walks more rows than a 16-bit prefix of 9 x 63 per row holds
