"""A numpy model of the left-right check, written from SURVEY.md Appendix A.4 (not from the kernels), that can NAME what it
decides: validate() is the check, census() counts, over the valid rectangle, every decision the check takes and every input
property its kernel forms are sensitive to, and VARIANTS are deliberately wrong versions of validate() -- the mistakes a
rewrite of csrc/k_lrcheck.hip is most likely to make.  tests/test_lr_states_cpu.py shows on the CPU that the cases of
tests/lr_cases.py make every state live and tell every variant from the oracle; no kernel is ever mutated.

A.4, per row: INVALID = (minD - 1) 16, M16 = 16 disp12MaxDiff, minX1 = max(minD + D, 0), maxX1 = W + min(minD, 0).
Pass 1 (x ascending in [minX1, maxX1), the VOTERS): skip INVALID; x2 = x - ((d + 8) >> 4); the slot x2 goes to the voter with
the strictly smallest cost, the first x among equals.  Pass 2 (same columns): x0 = x - (d >> 4), x1 = x - ((d + 15) >> 4); the
pixel is dropped iff BOTH slots are inside the row, hold a vote and that vote's disparity differs from d by more than M16.
A column outside [minX1, maxX1) that holds a disparity (the search computes column minD + D - 1 too) is a NON-VOTER: it
neither votes nor is checked; it lies left of the valid rectangle, so only its missing vote can be seen.
"""
import numpy as np

VARIANTS = {
    "second_plus16": "the second look-up at x - ((d + 16) >> 4)",
    "last_wins_tie": "the last voter wins a cost tie",
    "nonvoter_votes": "a non-voter's vote counts",
    "cost_int16": "costs compared as int16",
    "disp_wrap15": "disparities compared after wrapping into [-16384, 16384)",
    "thr_ge": "|d2 - d| >= M16 where > belongs",
    "thr_lax": "|d2 - d| > M16 + 1 (a >= M16 + 1 rewritten with the wrong sign)",
}

# per pixel of the valid rectangle (census() counts them there, under `keep`).  nonvoter_only: a look-up of a slot that holds a
# non-voter's vote and no other (it must read as empty); nonvoter_slot: also of a slot that a non-voter would win from its voters
PIXEL_STATES = ("lost_slot", "won_tie", "x0_eq_x1", "x0_ne_x1", "first_empty", "first_agrees", "second_agrees", "second_empty",
                "both_disagree", "diff_eq_M", "diff_eq_M1", "nonvoter_slot", "nonvoter_only")
# per row of the valid rectangle, whatever the column (who fills the slots)
ROW_STATES = ("nonvoter", "voters", "cost_ge_2_14", "cost_ge_2_15", "cost_ge_2_16")

_EMPTY = np.int64(2) ** 62
_CBIAS = 1 << 20


def _geometry(disp, W, minD, D):
    d = disp.astype(np.int64)
    assert d.ndim == 2 and d.shape[1] == W and W < 65536
    x = np.broadcast_to(np.arange(W, dtype=np.int64), d.shape)
    inv = (minD - 1) * 16
    votes = (x >= max(minD + D, 0)) & (x < W + min(minD, 0))
    return d, x, inv, votes


def _pass1(d, x, inv, votes, cost, W, nonvoters=False, last=False, cost16=False):
    """-> (win, voter, x2, mincost): win[y, s] = the column of slot s's winning voter (-1: no vote), voter[y, x], x2[y, x] =
    the slot x votes into, mincost[y, s] = the winning cost (as compared)"""
    H = d.shape[0]
    x2 = x - ((d + 8) >> 4)
    voter = (d != inv) & (x2 >= 0) & (x2 < W)
    if not nonvoters:
        voter = voter & votes
    c = cost.astype(np.int64)
    if cost16:
        c = c.astype(np.int16).astype(np.int64)
    order = (W - 1 - x) if last else x
    key = ((c + _CBIAS) << 16) | order
    slot = np.full(H * W, _EMPTY, np.int64)
    flat = np.arange(H, dtype=np.int64)[:, None] * W + x2
    np.minimum.at(slot, flat[voter], key[voter])
    slot = slot.reshape(H, W)
    full = slot != _EMPTY
    o = slot & 0xffff
    win = np.where(full, (W - 1 - o) if last else o, -1)
    return win, voter, x2, np.where(full, (slot >> 16) - _CBIAS, 0)


def _look(win, d, inv, xi, W):
    """the vote in slot xi -> (the slot is inside the row and holds a vote, that vote's disparity)"""
    inside = (xi >= 0) & (xi < W)
    wv = np.take_along_axis(win, np.clip(xi, 0, W - 1), 1)
    d2 = np.take_along_axis(d, np.clip(wv, 0, W - 1), 1)
    return inside & (wv >= 0) & (d2 > inv), d2


def _wrap15(v):
    return ((v + 16384) % 32768) - 16384


def validate(disp, cost, W, minD, D, M, variant=None):
    """disp int16 [rows, W] (x16), cost int [rows, W], M = disp12MaxDiff -> the checked plane (a copy).
    variant: None (A.4) or a key of VARIANTS."""
    assert variant is None or variant in VARIANTS, variant
    d, x, inv, votes = _geometry(disp, W, minD, D)
    win = _pass1(d, x, inv, votes, cost, W, nonvoters=variant == "nonvoter_votes", last=variant == "last_wins_tie",
                 cost16=variant == "cost_int16")[0]
    m16 = 16 * M
    f0, d20 = _look(win, d, inv, x - (d >> 4), W)
    f1, d21 = _look(win, d, inv, x - ((d + (16 if variant == "second_plus16" else 15)) >> 4), W)

    def bad(d2):
        diff = np.abs(_wrap15(d2) - _wrap15(d)) if variant == "disp_wrap15" else np.abs(d2 - d)
        return diff >= m16 if variant == "thr_ge" else diff > m16 + 1 if variant == "thr_lax" else diff > m16

    kill = votes & (d != inv) & f0 & bad(d20) & f1 & bad(d21)
    out = np.array(disp, np.int16)
    out[kill] = inv
    return out


def census(disp, cost, W, minD, D, M, rect, keep=None):
    """disp, cost: whole planes [H, W] as the search leaves them; rect = (x, y, w, h), the valid rectangle; keep: a bool plane --
    only its pixels are counted in the per-pixel states (the pixels a comparison of final maps can still see).
    -> {state: count} over PIXEL_STATES and ROW_STATES, plus "max_cost", the largest voter's cost."""
    d, x, inv, votes = _geometry(disp, W, minD, D)
    H = d.shape[0]
    rows = np.zeros((H, 1), bool); rows[rect[1]:rect[1] + rect[3]] = True
    inrect = rows & (x >= rect[0]) & (x < rect[0] + rect[2])
    if keep is not None:
        inrect = inrect & keep
    win, voter, x2, mincost = _pass1(d, x, inv, votes, cost, W)
    win_nv = _pass1(d, x, inv, votes, cost, W, nonvoters=True)[0]
    c = cost.astype(np.int64)
    x2c = np.clip(x2, 0, W - 1)
    mine = np.take_along_axis(win, x2c, 1) == x
    tied = np.zeros(H * W, np.int64)
    flat = np.arange(H, dtype=np.int64)[:, None] * W + x2c
    at_min = voter & (c == np.take_along_axis(mincost, x2c, 1))
    np.add.at(tied, flat[at_min], 1)
    tied = tied.reshape(H, W)
    m16 = 16 * M
    has = votes & (d != inv)
    xi0, xi1 = x - (d >> 4), x - ((d + 15) >> 4)
    f0, d20 = _look(win, d, inv, xi0, W)
    f1, d21 = _look(win, d, inv, xi1, W)
    g0, g1 = _look(win_nv, d, inv, xi0, W)[0], _look(win_nv, d, inv, xi1, W)[0]
    # the slot's vote would be a non-voter's if non-voters voted: alone in the slot, or ahead of its voters
    nv_wins = (win_nv >= 0) & ~np.take_along_axis(votes, np.clip(win_nv, 0, W - 1), 1)
    n0 = (xi0 >= 0) & (xi0 < W) & np.take_along_axis(nv_wins, np.clip(xi0, 0, W - 1), 1)
    n1 = (xi1 >= 0) & (xi1 < W) & np.take_along_axis(nv_wins, np.clip(xi1, 0, W - 1), 1)
    a0, a1 = np.abs(d20 - d), np.abs(d21 - d)
    b0, b1 = f0 & (a0 > m16), f1 & (a1 > m16)
    px = {
        "lost_slot": voter & ~mine,
        "won_tie": voter & mine & (np.take_along_axis(tied, x2c, 1) >= 2),
        "x0_eq_x1": has & (xi0 == xi1),
        "x0_ne_x1": has & (xi0 != xi1),
        "first_empty": has & ~f0,
        "first_agrees": has & f0 & ~b0,
        "second_agrees": has & b0 & f1 & ~b1,
        "second_empty": has & b0 & ~f1,
        "both_disagree": has & b0 & b1,
        "diff_eq_M": has & ((f0 & (a0 == m16)) | (f1 & (a1 == m16))),
        "diff_eq_M1": has & ((f0 & (a0 == m16 + 1)) | (f1 & (a1 == m16 + 1))),
        "nonvoter_slot": has & (n0 | n1),
        "nonvoter_only": has & ((g0 & ~f0) | (g1 & ~f1)),
    }
    out = {k: int((v & inrect).sum()) for k, v in px.items()}
    assert set(out) == set(PIXEL_STATES)
    vr = voter & rows
    out["nonvoter"] = int(((d != inv) & ~votes & rows).sum())
    out["voters"] = int(vr.sum())
    for bit in (14, 15, 16):
        out["cost_ge_2_%d" % bit] = int((vr & (c >= 1 << bit)).sum())
    out["max_cost"] = int(c[vr].max()) if vr.any() else 0
    return out
