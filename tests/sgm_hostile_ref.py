"""What the hostile StereoSGBM tests need beside the pairs of tests/sgm_hostile.py: the references (oracle/sgm_oracle.c; MODE_HH4:
sgm_hh4_ref; colour and preFilterCap: sgm_cn_ref), at_limit's P2, and R6 - R9 in NumPy with R7's tie rule and R9's quirk as
switches."""
import numpy as np

SAT = 32767


def limit_P2(Ls, Rs, D, minD, blockSize, preFilterCap=0):
    """32767 - the largest block cost of the frames (gray [n, H, W] or colour [n, H, W, 3]): the largest P2 at which none of
    them is refused"""
    import sgm_hh4_ref
    from oracle import oracle as orc
    p = orc.make_sgm_params(numDisparities=D, minDisparity=minD, blockSize=blockSize)
    cmax = max(int(sgm_hh4_ref.block_costs(np.ascontiguousarray(l), np.ascontiguousarray(r), p, preFilterCap)[1])
               for l, r in zip(Ls, Rs))
    return SAT - cmax


# ---- R6 - R9 in NumPy, with the two rules under test as switches ---------------------------------------------------------------
def select(S, W, minD, uniquenessRatio=10, disp12MaxDiff=1, larger_x_stays=True, scaled_invalid_votes=True):
    """orc_sgm_select restated: S uint16 [H, W1, D] -> (raw map int16 [H, W], events).  With both switches True this IS the
    oracle's selection (test_sgm_hostile_cpu.py compares the bytes).  larger_x_stays=False resolves R7's tie the other way (an
    equal minS replaces the vote); scaled_invalid_votes=False initialises the votes with a value below minD whatever minD is
    (R9 without its quirk).  events: the number of (row, right column) where a vote met a different winner with equal minS."""
    H, W1, D = S.shape
    INVALID = (minD - 1) * 16
    minX1 = max(minD + D, 0)
    uniq = uniquenessRatio if uniquenessRatio >= 0 else 10
    maxDiff = disp12MaxDiff if disp12MaxDiff > 0 else 1
    S = S.astype(np.int64)
    out = np.full((H, W), INVALID, np.int64)
    events = 0
    bd = S.argmin(axis=2)                                            # the first minimum
    mins = S.min(axis=2)
    dd = np.abs(np.arange(D)[None, None, :] - bd[:, :, None]) > 1
    rejected = ((S * (100 - uniq) < (mins * 100)[:, :, None]) & dd).any(axis=2) | (mins >= SAT)
    den = np.ones_like(mins); num = np.zeros_like(mins)
    inner = (bd > 0) & (bd < D - 1)
    yy, xx = np.nonzero(inner)
    sm, sp = S[yy, xx, bd[yy, xx] - 1], S[yy, xx, bd[yy, xx] + 1]
    den[yy, xx] = np.maximum(sm + sp - 2 * mins[yy, xx], 1)
    num[yy, xx] = (sm - sp) * 16
    t = num + den                                                     # C division: towards zero
    q = np.where(t >= 0, t // (den * 2), -((-t) // (den * 2)))
    d16 = np.where(inner, bd * 16 + q, bd * 16) + minD * 16
    for y in range(H):
        d2 = np.full(W, INVALID if scaled_invalid_votes else minD - 1, np.int64)
        c2 = np.full(W, SAT, np.int64)
        for xi in range(W1 - 1, -1, -1):
            if rejected[y, xi]:
                continue
            x = minX1 + xi
            x2 = x - int(bd[y, xi]) - minD
            if 0 <= x2 < W:
                m = int(mins[y, xi])
                if c2[x2] == m and d2[x2] != bd[y, xi] + minD:
                    events += 1
                if c2[x2] > m or (not larger_x_stays and c2[x2] == m):
                    c2[x2] = m; d2[x2] = bd[y, xi] + minD
            out[y, x] = d16[y, xi]
        for x in range(minX1, minX1 + W1):
            d1 = int(out[y, x])
            if d1 == INVALID:
                continue
            da, db = d1 >> 4, (d1 + 15) >> 4
            xa, xb = x - da, x - db
            if (0 <= xa < W and d2[xa] >= minD and abs(d2[xa] - da) > maxDiff and
                    0 <= xb < W and d2[xb] >= minD and abs(d2[xb] - db) > maxDiff):
                out[y, x] = INVALID
    return out.astype(np.int16), events


# ---- the references ----------------------------------------------------------------------------------------------------------
def resolve(params, Ls, Rs, D, minD, preFilterCap=0):
    """A parameter set of sgm_hostile_cases -> the oracle's keywords for these frames: numDisparities, minDisparity, and for
    at_limit (P2 None) P2 = limit_P2 of the frames and P1 = 3 P2 / 4."""
    kw = dict(params, numDisparities=D, minDisparity=minD)
    if kw.get("P2", 0) is None:
        kw["P2"] = limit_P2(Ls, Rs, D, minD, kw["blockSize"], preFilterCap)
        kw["P1"] = 3 * kw["P2"] // 4
    return kw


def volumes(L, R, paths, kw, preFilterCap=0):
    """-> (block costs, aggregated costs S) uint16 [H, W1, D] of a mode: the C oracle's for MODE_HH and MODE_SGBM on gray frames
    at preFilterCap 0, sgm_hh4_ref's otherwise"""
    import sgm_hh4_ref
    from oracle import oracle as orc
    p = orc.make_sgm_params(paths=paths, **kw)
    if paths != 4 and L.ndim == 2 and not preFilterCap:
        _, Cc, S = orc.sgm_stages(L, R, params=p)
        return Cc, S
    Cc, _ = sgm_hh4_ref.block_costs(np.ascontiguousarray(L), np.ascontiguousarray(R), p, preFilterCap)
    return Cc, sgm_hh4_ref.aggregate(Cc, p.P1, p.P2, sgm_hh4_ref.DIRS[paths])


def reference(L, R, paths, kw, preFilterCap=0):
    """The map the device must give, or ValueError (sgm_cn_ref.CostOverflow is one) where it must refuse the frame"""
    import sgm_cn_ref
    import sgm_hh4_ref
    from oracle import oracle as orc
    if paths == 4:
        return sgm_hh4_ref.sgm_compute(L, R, preFilterCap=preFilterCap, **kw)
    if L.ndim == 2 and not preFilterCap:
        return orc.sgm_compute(L, R, paths=paths, **kw)
    return sgm_cn_ref.sgm_compute_cn(L, R, preFilterCap=preFilterCap, paths=paths, **kw)
