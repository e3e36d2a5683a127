"""CPU check of what GroupSelectRec::finish (rt-depth-map_amd/csrc/rtdm_select.h) computes, against the plain rule of the
oracle (oracle/bm_oracle.c:175-191): the FIRST argmin, and rejection iff some index outside [a-1, a+1] has
sad <= T = minsad + minsad * ratio / 100.

  * the neighbour group of test (B) is masked by its threshold (0 when a-1 and a+1 lie in the winner's group):
    max(0 - sad, 0) = 0 with saturating u16 arithmetic, the same as masking its four terms;
  * the bound the f16 reading of the group minima (sel_pk_min3_h) rests on: window sums below 0x7C00 for every ring form,
    and positive finite f16 ordered as their bit patterns.
"""
import numpy as np
import pytest

from test_select_identity import reject_plain, vectors


def sub_sat(a, b):
    return max(a - b, 0)


def reject_group_select_rec(sad, ratio):
    """GroupSelectRec::finish: first group of the smallest minimum, first index of it inside the group, (A) over the group
    minima + (B) over the one or two groups."""
    D = len(sad)
    NG = D // 8
    gmin = sad.reshape(NG, 8).min(axis=1)
    gs = int(np.argmin(gmin)); m1 = int(gmin[gs])
    grp = sad[8 * gs:8 * gs + 8]
    e = int(np.argmin(grp))
    a = 8 * gs + e
    T = min(m1 + m1 * ratio // 100, 32766); T1 = T + 1
    # (A): two saturating halves over the group minima (even groups low, odd groups high)
    za = [0, 0]
    for g in range(NG):
        za[g % 2] = min(za[g % 2] + sub_sat(T1, int(gmin[g])), 65535)
    zg = za[0] + za[1]
    has_n, has_p = a > 0, a + 1 < D
    nbq = gs - 1 if (e == 0 and has_n) else gs + 1 if (e == 7 and has_p) else gs
    has_nb = nbq != gs
    t1nb = T1 if has_nb else 0                               # the threshold mask of the neighbour group
    nbg = sad[8 * nbq:8 * nbq + 8]
    # the kernel adds the two groups' terms pairwise per register before the chain; saturating sums of non-negative terms
    # are order independent, so one chain per half models it
    zb = [0, 0]
    for i in range(8):
        zb[i % 2] = min(zb[i % 2] + sub_sat(T1, int(grp[i])), 65535)
        zb[i % 2] = min(zb[i % 2] + sub_sat(t1nb, int(nbg[i])), 65535)
    z = zb[0] + zb[1]
    term = lambda v: sub_sat(T1, int(v))
    want = term(m1) + (term(sad[a - 1]) if has_n else 0) + (term(sad[a + 1]) if has_p else 0)
    wantg = term(m1) + (term(gmin[nbq]) if has_nb else 0)
    return (z + zg) != (want + wantg), a, m1


@pytest.mark.parametrize("D", [16, 32, 48, 64, 96, 128])
def test_group_select_rec_equals_the_plain_rule(D):
    rng = np.random.default_rng(2000 + D)
    for ratio in (0, 1, 10, 25, 100, 400):
        for sad in vectors(rng, D, 1200):
            rej, a, m = reject_group_select_rec(sad, ratio)
            want, wa, wm, _ = reject_plain(sad, ratio)
            assert (a, m) == (wa, wm)
            assert rej == want, (D, ratio, sad.tolist())


def test_bounds_of_the_switches():
    # every ring form: cap <= 63 (rtdm_bm_create) and 2 cap w^2 <= 32766 (ring_form) => w <= 15
    assert max(2 * 63 * w * w for w in range(1, 17, 2) if 2 * 63 * w * w <= 32766) < 0x7C00
    # positive finite f16 (u16 < 0x7C00, denormals included) sort as their bit patterns do
    h = np.arange(0x7C00, dtype=np.uint16).view(np.float16)
    assert np.all(np.isfinite(h)) and np.all(np.diff(h.astype(np.float64)) > 0)
