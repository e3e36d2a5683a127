"""The paired ring search k_search_ring<64, 9, 4> with the next row's LDS reads issued one step ahead (RingCfg::PREFETCH,
k_search_ring.hip) against the oracle, bit for bit.  A wrong row -- the read-ahead taken from the wrong staging slot, or the
wrong register set consumed behind a group, trip or strip boundary -- changes the window sums of every later row of the strip.

Shapes by STEPS PER STRIP (output rows + 8): 20, 21, 24, 25, 28, 40, 41, 44, 60 and 61, every one of them at n = 1 (the
instantiation with the border workgroups in its grid) and at n = 16 (tile-only); W = 128 (one partly active tile) and
W = 200 (ragged last tile), but for the long strips at n = 1, which only wide frames get.  Up to 24 steps a frame is one strip (H = steps); above, the strip model hands out such strips only
in frames of many strips -- a few hundred rows at n = 16, frames as wide as the headline's at n = 1 -- and
tests/test_ring_prefetch_cpu.py pins how it cuts every shape used here.  Batches of 2048 small frames add every length as a
single strip.  Content: noise with every default threshold on (uniqueness, texture, left-right check, speckle) and `ties`,
where the first-minimum rule turns a wrong row into a wrong winner; the default speckle filter empties noise frames this
small, so noise runs without it as well, and `edges`, which survives every default threshold, runs with all of them on: each
of these runs has a floor of valid pixels.  A batch repeats two distinct frames; every copy is compared with its source, the
two sources with the oracle."""
import numpy as np
import pytest

import hostile_pairs as hp
from conftest import load
from test_ring_prefetch_cpu import D, MULTI_STRIP, ONE_STRIP, WS

pytestmark = pytest.mark.gpu

VARIANT = "fast_ring4_qsad"


@pytest.fixture(scope="module")
def pkg():
    import torch
    assert torch.cuda.is_available(), "the -m gpu suite needs an MI355X"
    return load()


def run(pkg, L2, R2, n, **kw):
    """The two frames of L2, R2 [2, H, W] repeated to a batch of n, through one handle and ONE call (the strip model stays in
    charge): one frame through compute, more through compute_device.  -> int16 [n, H, W]"""
    import torch
    _, H, W = L2.shape
    m = pkg.HIPMatcher(numOfDisparities=D, blockSize=WS, width=W, height=H, max_batch=n, **kw)
    try:
        if n == 1:
            got = m.compute(L2[0], R2[0])[None]
        else:
            dL = torch.from_numpy(L2).cuda().repeat(n // 2, 1, 1)
            dR = torch.from_numpy(R2).cuda().repeat(n // 2, 1, 1)
            dD = torch.full((n, H, W), 12345, dtype=torch.int16, device="cuda")
            m.compute_device(dL, dR, dD, torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            bad = (dD != dD[:2].repeat(n // 2, 1, 1)).flatten(1).any(1).nonzero().flatten()   # every copy against its source
            assert bad.numel() == 0, "%d frames differ from their source, first %d" % (bad.numel(), int(bad[0]))
            got = dD[:2].cpu().numpy()
        assert m.search_variant == VARIANT, m.search_variant
        return got
    finally:
        m.close()


def same(got, want, what):
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError("%s: %d pixels differ, first (y, x) = %s got %d want %d" % (what, len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])]))


def check(pkg, oracle, L2, R2, n, what, **kw):
    got = run(pkg, L2, R2, n, **kw)
    valid = 0
    for i in range(min(n, 2)):
        want = oracle.bm_compute(L2[i], R2[i], numDisparities=D, blockSize=WS, **kw)
        same(got[i], want, "%s n=%d %s frame %d" % (what, n, kw, i))
        valid += int((want != -16).sum())
    return valid


FLOOR = 100       # valid pixels per compared frame below which a run compares next to nothing


def both_contents(pkg, oracle, W, H, n):
    frames = min(n, 2)
    L, R = hp.noise_bands(7 * H + W + n, W, H, D, 2)
    check(pkg, oracle, L, R, n, "noise %dx%d" % (W, H))                              # every default threshold on
    # (in frames this small the default speckle filter takes every pixel of the noise; without it the search's own output shows)
    valid = check(pkg, oracle, L, R, n, "noise %dx%d" % (W, H), speckleWindowSize=0)
    assert valid >= FLOOR * frames, "the oracle filters the noise frames almost entirely (%d valid): nothing is compared" % valid
    L, R = hp.make_n("ties", H + n, 2, W, H, D, 0, WS)
    valid = check(pkg, oracle, L, R, n, "ties %dx%d" % (W, H), uniquenessRatio=0, textureThreshold=0, speckleWindowSize=0, disp12MaxDiff=-1)
    assert valid >= FLOOR * frames, "ties %dx%d: %d valid pixels" % (W, H, valid)
    # every default threshold on, with content that survives them (the uniqueness test takes most of `ties`, by construction)
    L, R = hp.make_n("edges", H + n, 2, W, H, D, 0, WS)
    valid = check(pkg, oracle, L, R, n, "edges %dx%d, thresholds on" % (W, H))
    assert valid >= FLOOR * frames, "edges %dx%d with the default thresholds: %d valid pixels" % (W, H, valid)


def ident(case):
    W, H, n, strips, rs = case
    return "%dx%d-n%d-%dx%dsteps" % (W, H, n, strips, rs + WS - 1)


@pytest.mark.parametrize("case", ONE_STRIP, ids=ident)
def test_steps_per_strip(pkg, oracle, case):
    W, H, n, strips, rs = case
    assert strips == 1 and H == rs + WS - 1
    both_contents(pkg, oracle, W, H, n)


@pytest.mark.parametrize("case", MULTI_STRIP, ids=ident)
def test_strips_that_start_inside_the_frame(pkg, oracle, case):
    W, H, n, strips, rs = case
    assert strips >= 2
    both_contents(pkg, oracle, W, H, n)
