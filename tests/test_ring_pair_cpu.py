"""The row step of the paired ring layout (k_search_ring.hip: ring_step_pair, RingCfg::PAIR), restated in numpy on one wave's
staged copy: per lane and quad-group the two shared pieces are summed once, each column adds its one-byte masked piece on top of
its own prefix sum, and the shared sum joins both with 32-bit additions of the packed 16-bit halves.  Checked against brute-force
9-byte SADs and 9-row window sums, with the prefix rings rebased as the kernel rebases them."""
import numpy as np
import pytest

D, WS, R = 64, 9, 4
W1 = WS + 1
LWD, RWD = 11, 27                    # dwords of the wave's copy of the left / right row
TRIP = 20                            # rows per trip of the unrolled row loop: whole rounds of the ring and whole groups of four


def _qsad(win, ref, acc, masked):
    """v_qsad_pk_u16_u8 / v_mqsad_pk_u16_u8 on arrays: win [..., 8] bytes, ref [..., 4] bytes, acc [..., 4] -> [..., 4];
    masked: reference bytes that are zero are skipped."""
    out = acc.astype(np.int64).copy()
    for s in range(4):
        d = np.abs(win[..., s:s + 4].astype(np.int64) - ref.astype(np.int64))
        if masked:
            d = np.where(ref == 0, 0, d)
        out[..., s] += d.sum(-1)
    return out


def _row_pieces(Lc, Rc):
    """One row of one wave.  Lc [44], Rc [108]: the copy's bytes.  Returns e1, e2, sh [8 q, 8 h, 2 gi, 4] with zero accumulators:
    the one-byte pieces of columns x0 and x0 + 1 and the shared sum."""
    q = np.arange(8)[:, None, None, None]
    h = np.arange(8)[None, :, None, None]
    gi = np.arange(2)[None, None, :, None]
    byte = np.arange(8)[None, None, None, :]
    win = [Rc[4 * (q + 2 * h + gi + k) + byte] for k in range(4)]                     # the right windows gi .. gi + 3 of the lane
    l = [np.broadcast_to(Lc[4 * (q + k) + byte[..., :4]], (8, 8, 2, 4)).copy() for k in range(4)]
    lf, ll = l[0].copy(), l[3].copy()
    lf[..., :3] = 0                                                                    # l[0] & 0xff000000
    ll[..., 1:] = 0                                                                    # l[3] & 0x000000ff
    zero = np.zeros((8, 8, 2, 4), np.int64)
    sh = _qsad(win[2], l[2], _qsad(win[1], l[1], zero, False), False)
    return _qsad(win[0], lf, zero, True), _qsad(win[3], ll, zero, True), sh


def _brute(Lc, Rc):
    """SAD[c, i] of the 9-byte windows centred on copy byte 7 + c, c = 0 .. 31 (the 16 pairs' columns), i = 0 .. 63."""
    out = np.zeros((32, D), np.int64)
    for c in range(32):
        for i in range(D):
            a = Lc[7 + c - R:7 + c + R + 1].astype(np.int64)
            b = Rc[7 + c - R + i:7 + c + R + 1 + i].astype(np.int64)
            out[c, i] = np.abs(a - b).sum()
    return out


def _as_columns(v):
    """[8 q, 8 h, 2 gi, 4 s] of column j of the pairs -> [8 q, 64]: index i = 8 h + 4 gi + s."""
    return v.reshape(8, D)


def _rows(rng, n, cap, worst):
    lo, hi = 1, 2 * cap + 1                                  # biased prefiltered bytes
    if worst:                                                # every byte pair differs by 2 cap: the prefix sums grow as fast as they can
        return np.full((n, 4 * LWD), lo, np.uint8), np.full((n, 4 * RWD), hi, np.uint8)
    return rng.integers(lo, hi + 1, (n, 4 * LWD), dtype=np.uint8), rng.integers(lo, hi + 1, (n, 4 * RWD), dtype=np.uint8)


@pytest.mark.parametrize("cap", (31, 63))
def test_row_step_equals_the_brute_force_sads_of_both_columns(cap):
    rng = np.random.default_rng(cap)
    Lr, Rr = _rows(rng, 6, cap, False)
    Lr[2, 12:20] = 1                                         # (bytes at the bias: a ZERO byte would be skipped, these must not be)
    for Lc, Rc in zip(Lr, Rr):
        e1, e2, sh = _row_pieces(Lc, Rc)
        want = _brute(Lc, Rc)
        assert np.array_equal(_as_columns(e1 + sh), want[[4 * q for q in range(8)]])       # pair q: copy bytes 7 + 4 q and 8 + 4 q
        assert np.array_equal(_as_columns(e2 + sh), want[[4 * q + 1 for q in range(8)]])


def _pack(v):
    """[..., 4] sums -> [..., 2] uint32: two 16-bit halves per dword, as the quad-SAD instructions write them."""
    v = v.astype(np.uint64)
    return ((v[..., 0::2] & 0xffff) | ((v[..., 1::2] & 0xffff) << 16)).astype(np.uint32)


def _unpack(p):
    return np.stack([p[..., 0] & 0xffff, p[..., 0] >> 16, p[..., 1] & 0xffff, p[..., 1] >> 16], -1).astype(np.int64)


def prefix_ring_window_sums(Lr, Rr, rebase, strict=True):
    """The packed prefix rings of both columns of the pairs walked down the rows Lr [rows, 44], Rr [rows, 108] (one wave's
    copies, biased bytes), rebased every `rebase` trips as the kernel rebases them (None: never).  Returns (got, want):
    the window sums read from the rings and the exact ones, [rows - 8, 2, 8, 8, 2, 4].  strict: assert on the way that no
    16-bit half overflows and every window sum is exact."""
    rows = len(Lr)
    H1, H2 = [], []                                          # the rows' horizontal SADs per column, exact
    P = np.zeros((2, W1, 8, 8, 2, 2), np.uint32)             # [column of the pair][ring slot][q][h][gi][dword]: packed prefix sums
    since = 0
    got, wanted = [], []
    for t in range(rows):
        K, KP, KO = t % W1, (t - 1) % W1, (t + 1) % W1
        if t % TRIP == 0 and rebase is not None:
            since += 1
            if since > rebase:                               # a trip starts on slot 0; slot 1 holds the oldest live prefix sum
                since = 1
                for j in range(2):
                    base = P[j, 1].copy()
                    for k in range(1, W1):
                        P[j, k] = P[j, k] - base             # 32-bit subtractions of the packed halves
        e1, e2, sh = _row_pieces(Lr[t], Rr[t])
        H1.append(e1 + sh); H2.append(e2 + sh)
        shp = _pack(sh)
        row_got, row_want = [], []
        for j, e in ((0, e1), (1, e2)):
            acc = _unpack(P[j, KP]) + e                      # v_mqsad on top of the column's previous prefix sum
            if strict:
                assert acc.max() < 65536
            P[j, K] = _pack(acc) + shp                       # v_add_u32 per dword: no carry may cross the halves
            if strict:
                assert np.array_equal(_unpack(P[j, K]), acc + sh), "a 16-bit half overflowed at row %d" % t
            S = P[j, K] - P[j, KO]                           # v_sub_u32 per dword
            if t >= WS - 1:
                want = sum((H1, H2)[j][t - WS + 1:t + 1])
                if strict:
                    assert np.array_equal(_unpack(S), want), (t, j)
                row_got.append(_unpack(S)); row_want.append(want)
        if t >= WS - 1:
            got.append(np.stack(row_got)); wanted.append(np.stack(row_want))
    return np.stack(got), np.stack(wanted)


@pytest.mark.parametrize("cap,rows,worst", [(31, 230, False), (63, 104, False), (31, 230, True), (63, 104, True)])
def test_packed_prefix_rings_give_the_window_sums_across_rebases(cap, rows, worst):
    # the host's arithmetic: ring_rows_cap / TRIP trips between two rebases (k_search_ring.hip)
    rows_cap = 65535 // (WS * 2 * cap) - WS - 6
    rebase = rows_cap // TRIP
    assert rebase > 0 and rows > 2 * rebase * TRIP           # the strip crosses at least two rebases
    rng = np.random.default_rng(100 + cap)
    Lr, Rr = _rows(rng, rows, cap, worst)
    got, want = prefix_ring_window_sums(Lr, Rr, rebase)
    assert got.shape[0] == rows - WS + 1 and np.array_equal(got, want)
