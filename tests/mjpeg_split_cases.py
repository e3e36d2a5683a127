"""Streams and figures shared by the tests of the split MJPEG decoder (test_mjpeg_split_cpu.py, test_gpu_mjpeg_split.py)."""
import numpy as np

import mjpeg_ref as ref
import mjpeg_synth as synth


def entropy_len(stream):
    lo, hi = ref.entropy_range(stream)
    return hi - lo


def plan(length, S):
    """mjpeg_split_plan of rtdm_mjpeg.h: (subsequences, their size) of `length` entropy bytes when S bytes are asked for"""
    sp = max(S, -(-length // 1024))
    return -(-length // sp), sp


def without_dri(letter):
    """the streams of class `letter` of mjpeg_synth, written with ri = 0 (the classes name their own restart intervals)"""
    real = synth.write

    def write(*a, **kw):
        kw["ri"] = 0
        return real(*a, **kw)

    synth.write = write
    try:
        items = synth.class_streams(letter)
    finally:
        synth.write = real
    seen, out = set(), []
    for label, s in items:                       # class d writes one content with seven restart intervals
        if s not in seen:
            seen.add(s)
            out.append((label, s))
    return out


SATURATING_STEPS = np.array([2047] * 18 + [-2047] * 50 + [2047] * 52)


def saturating_dc_stream():
    """960 x 8, 2x1, unit quantisers: the DC levels of every component climb in steps of 2047 beyond +32767, fall beyond -32768
    and climb again.  The decoder's predictor saturates on the way (the encoder's does not), so from there on it is the clamp
    that decides what the coefficients are."""
    n = 60
    rng = np.random.default_rng(77)
    comps = [np.zeros((1, 2 * n, 64), np.int64), np.zeros((1, n, 64), np.int64), np.zeros((1, n, 64), np.int64)]
    comps[0][0, :, 0] = np.cumsum(SATURATING_STEPS)
    comps[1][0, :, 0] = np.cumsum(-SATURATING_STEPS[:n])
    comps[2][0, :, 0] = np.cumsum(np.roll(SATURATING_STEPS, 9)[:n])
    for c in comps:
        c[0, :, 1:6] = rng.integers(-3, 4, (c.shape[1], 5))
    return synth.write(16 * n, 8, "2x1", comps, synth.unit_quant())


NOISE_W, NOISE_H = 264, 96


def noise_frame(seed, lo, hi):
    """A 264 x 96 gray frame without restart intervals whose entropy data is lo < length <= hi bytes long (hi - lo >= 8): the
    first blocks hold noise (8 to 40 coefficients of up to five bits at random places), as many of them as fit; behind them
    coefficients of +1, three bits each with the standard tables, bring the length into the window.  Inside mjpeg_synth's
    domain by construction (into_domain)."""
    assert hi - lo >= 8
    rng = np.random.default_rng(seed)
    by, bx = NOISE_H // 8, NOISE_W // 8
    nblk = by * bx
    q = np.ones(64, np.int64)
    dense = np.zeros((nblk, 64), np.int64)
    for b in range(nblk):
        nz = int(rng.integers(8, 41))
        dense[b, rng.choice(np.arange(1, 64), nz, replace=False)] = rng.integers(1, 32, nz) * rng.choice([-1, 1], nz)
        dense[b, 0] = int(rng.integers(-200, 200))
    dense = synth.into_domain(dense.reshape(by, bx, 64), q).reshape(nblk, 64)

    def stream(m, k):
        b = np.zeros((nblk, 64), np.int64)
        b[:m] = dense[:m]
        tail = b[m:, 1:].reshape(-1)
        tail[:k] = 1
        b[m:, 1:] = tail.reshape(nblk - m, 63)
        return synth.write(NOISE_W, NOISE_H, "gray", [b.reshape(by, bx, 64)], {0: q})

    a, z = 0, nblk - 8                               # the most noise blocks that stay at or below lo
    assert entropy_len(stream(a, 0)) <= lo < entropy_len(stream(z, (nblk - z) * 63)), (lo, hi)
    while a < z:
        mid = (a + z + 1) // 2
        if entropy_len(stream(mid, 0)) <= lo:
            a = mid
        else:
            z = mid - 1
    m, k, goal = a, 0, (lo + hi + 1) // 2
    for _ in range(24):
        s = stream(m, k)
        n = entropy_len(s)
        if lo < n <= hi:
            return s
        k = min(max(0, k + -(-(goal - n) * 8 // 3)), (nblk - m) * 63)
    raise AssertionError("no frame of %d < length <= %d" % (lo, hi))
