"""Every route of the StereoBM search stage (plan_search in k_search.hip; the table of DESIGN.md, "K2: routes") against the
oracle, bit for bit: a single frame through compute -- the border columns in the tile kernel's grid or behind it -- and a
batch of 16 through compute_device, where every border launch of its own runs on the side stream.  Each row is the smallest
frame at which its route exists (tests/test_search_plan_cpu.py pins what is planned for it)."""
import functools

import numpy as np
import pytest

from conftest import load
from test_gpu_dslice import assert_same

pytestmark = pytest.mark.gpu

N = 16
# W, H, D, w, minD, cap, legacy, variant
ROWS = [(300, 80, 64, 9, 0, 31, 0, "fast_ring4_qsad"),       # ROWS fused / on the side stream
        (560, 90, 256, 15, 0, 15, 0, "fast_ring16_qsad"),    # DISP fused (D = 256 at n = 1) / ROWS on the side stream
        (250, 66, 32, 9, 0, 63, 0, "fast_ring_qsad"),        # DISP fused (three waves) / DISP on the side stream
        (300, 80, 64, 9, 0, 63, 0, "fast_ring4_qsad"),       # DISP behind the tiles (four waves) / on the side stream
        (300, 80, 80, 9, 0, 31, 0, "fast_qsad"),             # DISP in k_search_fast's grid / on the side stream
        (300, 80, 64, 17, 0, 31, 0, "fast_qsad"),            # the same with five window pieces
        (200, 50, 64, 23, 0, 30, 0, "fast_qsad"),            # two generic column ranges behind the tiles, at every n
        (300, 80, 64, 9, -7, 31, 1, "fast_ring4_qsad"),      # DISP + LEGACY behind the tiles / on the side stream
        (300, 90, 64, 25, 0, 31, 0, "generic_u16"),          # generic tiles over the whole range
        (400, 80, 272, 9, 0, 31, 0, "generic_dslice_u16")]


@pytest.fixture(scope="module")
def pkg():
    import torch                         # torch first: it brings its own HIP runtime and must initialise before ours
    assert torch.cuda.is_available(), "the -m gpu suite needs an MI355X"
    return load()


@functools.lru_cache(maxsize=None)
def _stream(synth, W, H, D, w):
    L, R = synth.make_stream(500 + D + w, N, W, H, min(D, 256))
    L.setflags(write=False); R.setflags(write=False)
    return L, R


@functools.lru_cache(maxsize=None)
def _want(oracle, synth, row, frame, legacy):
    W, H, D, w, minD, cap = row[:6]
    L, R = _stream(synth, W, H, D, w)
    oracle.set_legacy_right_clamp(bool(legacy))
    try:
        want = oracle.bm_compute(L[frame], R[frame], numDisparities=D, blockSize=w, minDisparity=minD, preFilterCap=cap, nthreads=8)
    finally:
        oracle.set_legacy_right_clamp(False)
    want.setflags(write=False)
    return want


def _check(oracle, synth, row, frame, got, what):
    minD, legacy = row[4], row[6]
    want = _want(oracle, synth, row[:7], frame, legacy)
    live = float((want != (minD - 1) * 16).mean())
    print("%s frame %d: %.3f of the oracle's pixels are not FILTERED" % (what, frame, live))
    assert live > 0.15
    assert_same(got, want, "%s frame %d" % (what, frame))
    if legacy:                            # the 3.x rule is live on this frame: the plain rule gives another one
        assert (want != _want(oracle, synth, row[:7], frame, 0)).any()


def _matcher(pkg, row, n):
    W, H, D, w, minD, cap, legacy = row[:7]
    return pkg.HIPMatcher(numOfDisparities=D, blockSize=w, minDisparity=minD, preFilterCap=cap, width=W, height=H, max_batch=n,
                          legacy_right_clamp=legacy)


@pytest.mark.parametrize("row", ROWS, ids=lambda r: "%dx%d-D%d-w%d-minD%d-cap%d-legacy%d" % r[:7])
def test_single_frame(pkg, oracle, synth, row):
    W, H, D, w = row[:4]
    L, R = _stream(synth, W, H, D, w)
    m = _matcher(pkg, row, 1)
    got = m.compute(L[0], R[0])
    variant = m.search_variant
    m.close()
    assert variant == row[7]
    _check(oracle, synth, row, 0, got, "n=1 %s" % (row[:7],))


@pytest.mark.parametrize("row", ROWS, ids=lambda r: "%dx%d-D%d-w%d-minD%d-cap%d-legacy%d" % r[:7])
def test_batch_of_16(pkg, oracle, synth, row):
    import torch
    W, H, D, w = row[:4]
    L, R = _stream(synth, W, H, D, w)
    dL, dR = torch.from_numpy(np.array(L)).cuda(), torch.from_numpy(np.array(R)).cuda()
    dD = torch.empty((N, H, W), dtype=torch.int16, device="cuda")
    m = _matcher(pkg, row, N)
    m.compute_device(dL, dR, dD, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    variant = m.search_variant
    got = dD.cpu().numpy()
    m.close()
    assert variant == row[7]
    for frame in (0, N - 1):
        _check(oracle, synth, row, frame, got[frame], "n=%d %s" % (N, row[:7]))
