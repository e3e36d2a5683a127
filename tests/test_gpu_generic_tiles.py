"""Every instantiation of the two generic search kernels (k_search_generic and k_search_dslice in k_search_generic.hip: sum
type uint16 / uint32 x tile width 64 / 8) against the oracle, bit for bit, at the smallest shapes that reach it; the
legacy_right_clamp wrap rule, which the shared row staging holds for both, through both; and the border columns behind the
packed kernels, which come back to launch_search_generic as two column ranges.

The 8-column tiles run when at most 16 columns are searched; with disp12MaxDiff = -1 the searched range is the valid one,
W - 2r - D + 1 columns.  rtdm_debug_disparity_slice is reset in `finally` everywhere (test_gpu_dslice.forced_slice)."""
import functools

import pytest

from conftest import load
from test_gpu_dslice import assert_same, forced_slice, run

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    import torch                         # torch first: it brings its own HIP runtime and must initialise before ours
    assert torch.cuda.is_available(), "the -m gpu suite needs an MI355X"
    return load()


@functools.lru_cache(maxsize=None)
def _pair(synth, W, H, D):
    return synth.make_pair(synth.STREAM_SEED + 1, W, H, D)


# (variant, D, preFilterCap, width that leaves 10 searched columns, forced slice width); blockSize 25 throughout
ROWS = [("generic_u16", 64, 31, 97, 0),
        ("generic_u32", 64, 63, 97, 0),
        ("generic_dslice_u16", 64, 31, 97, 16),
        ("generic_dslice_u32", 64, 63, 97, 16),
        ("generic_dslice_u32", 272, 63, 305, 0)]       # unforced: D > 256
# the 8-column tiles, then the 64-column tiles of the D = 64 rows (113 searched columns: two tiles)
CASES = [r + (r[3],) for r in ROWS] + [r + (200,) for r in ROWS[:4]]


@pytest.mark.parametrize("tex,uniq", [(0, 0), (10, 10)])
@pytest.mark.parametrize("variant,D,cap,narrow_W,dt,W", CASES)
def test_every_instantiation(pkg, oracle, synth, variant, D, cap, narrow_W, dt, W, tex, uniq):
    H = 40
    L, R = _pair(synth, W, H, D)
    kw = dict(numDisparities=D, blockSize=25, preFilterCap=cap, textureThreshold=tex, uniquenessRatio=uniq,
              speckleWindowSize=0, disp12MaxDiff=-1)
    with forced_slice(pkg, dt):
        got, want, got_variant = run(pkg, oracle, L, R, **kw)
    assert got_variant == variant
    valid = int((want != -16).sum())
    print("%s D=%d W=%d tex=%d uniq=%d: %d valid pixels" % (variant, D, W, tex, uniq, valid))
    if W == narrow_W:                                   # 10 columns x 16 rows are searched
        assert valid >= 150
    assert_same(got, want, "%s D=%d cap=%d W=%d tex=%d uniq=%d" % (variant, D, cap, W, tex, uniq))


@pytest.mark.parametrize("minD", [0, -7])
@pytest.mark.parametrize("dt", [0, 16])
def test_legacy_right_clamp_through_both_kernels(pkg, oracle, synth, dt, minD):
    # minDisparity 0: the wrap is met only in the columns the left-right check searches right of the valid ones;
    # below 0 valid pixels see the next row too, and the oracle's own two clamp rules give different frames
    D, W, H = 64, 200, 40
    L, R = _pair(synth, W, H, D)
    kw = dict(numDisparities=D, blockSize=25, preFilterCap=31, minDisparity=minD)
    with forced_slice(pkg, dt):
        got, want, variant = run(pkg, oracle, L, R, legacy=1, **kw)
    assert variant == ("generic_dslice_u16" if dt else "generic_u16")
    assert_same(got, want, "legacy dt=%d minD=%d" % (dt, minD))
    assert (want != (minD - 1) * 16).any()
    if minD < 0:
        assert (want != oracle.bm_compute(L, R, nthreads=8, **kw)).any()


@pytest.mark.parametrize("D,cap,W,H", [(32, 15, 120, 40), (64, 30, 200, 50)])
def test_border_columns_behind_the_packed_kernels(pkg, oracle, synth, D, cap, W, H):
    # blockSize 23: the packed kernels take the interior, no border kernel covers windows above 21, so the border columns
    # come back to launch_search_generic as two column ranges
    L, R = _pair(synth, W, H, D)
    got, want, variant = run(pkg, oracle, L, R, numDisparities=D, blockSize=23, preFilterCap=cap)
    assert variant.startswith("fast"), variant
    print("border D=%d: %.3f valid" % (D, (want != -16).mean()))
    assert (want != -16).mean() > 0.15
    assert_same(got, want, "border D=%d cap=%d" % (D, cap))
