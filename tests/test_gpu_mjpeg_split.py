"""k_mjpeg_huff_split on the device: a frame without restart intervals cut among up to 1024 lanes of one workgroup (DESIGN.md
section 4.12).  Its reference is the one-lane loop (split = 0 on the same handle) and, through it, the images Pillow decoded from
the stored streams and mjpeg_ref.py; the tolerance is zero.  The shapes are the edges of the lane count and the cuts, not large
frames: test_mjpeg_split_cpu.py has run the same passes over the same kinds of stream on the CPU, under the sanitizers too."""
import numpy as np
import pytest

import mjpeg_ref as ref
import mjpeg_synth as synth
from conftest import load
from mjpeg_split_cases import NOISE_H, NOISE_W, entropy_len, noise_frame, plan, saturating_dc_stream

pytestmark = pytest.mark.gpu

STD = ref.std_tables()
NO_DRI = [n for n in ref.FIXTURES if ref.parse(ref.load_fixture(n)[0], STD).ri == 0]
DEFAULT = 64             # MJ_SPLIT_DEFAULT of rtdm_mjpeg.h


@pytest.fixture(scope="module")
def pkg():
    import torch                         # torch first: it brings its own HIP runtime and must initialise before ours
    assert torch.cuda.is_available()
    return load()


@pytest.fixture(scope="module")
def dec(pkg):
    d = pkg.HIPMJPEGDecoder(NOISE_W, NOISE_H, max_batch=4, max_stream_bytes=65536)
    yield d
    d.close()


def _batch(dec, streams, W, H, pad_row=0, pad_frame=0):
    """decode_batch into a tensor whose rows and frames are padded and pre-filled with 0xA5 -> (frames, padding intact, status)"""
    import torch
    n, row = len(streams), W * 3 + pad_row
    flat = torch.full((n, H * row + pad_frame), 0xA5, dtype=torch.uint8, device="cuda")
    view = torch.as_strided(flat, (n, H, W, 3), (H * row + pad_frame, row, 3, 1))
    status = torch.full((n,), 77, dtype=torch.int32, device="cuda")
    dec.decode_batch(streams, out=view, status=status)
    torch.cuda.synchronize()
    host = flat.cpu().numpy()
    img = np.lib.stride_tricks.as_strided(host, (n, H, W, 3), (host.strides[0], row, 3, 1))
    mask = np.ones(host.shape, bool)
    np.lib.stride_tricks.as_strided(mask, (n, H, W * 3), (mask.strides[0], row, 1))[...] = False
    return img.copy(), bool((host[mask] == 0xA5).all()), status.cpu().numpy()


def test_a_new_handle_splits_by_default_and_checks_the_setting(pkg):
    B = pkg.binding
    d = pkg.HIPMJPEGDecoder(64, 48)
    assert d.split == DEFAULT and d.split_stats() == (0, 0, 0)
    for v in (0, 8, 65536, 37):
        d.split = v
        assert d.split == v
    d.split = -1
    assert d.split == DEFAULT
    d.split = None
    assert d.split == DEFAULT
    for v in (1, 7, 65537, -2):
        with pytest.raises(B.RtdmError) as e:
            d.split = v
        assert e.value.status == -1 and d.split == DEFAULT
    d.close()
    d = pkg.HIPMJPEGDecoder(64, 48, split=0)
    assert d.split == 0
    d.close()


@pytest.mark.parametrize("name", NO_DRI)
def test_fixtures_equal_pillow_at_every_setting(dec, name):
    stream, rgb, _ = ref.load_fixture(name)
    n = entropy_len(stream)
    dec.split = 0
    before = dec.split_stats()
    plain = dec.decode(stream)
    assert np.array_equal(plain, rgb)
    assert dec.split_stats() == before                       # off: the counters stay where they were
    for S in (8, 16, 64, None):
        dec.split = S
        size = DEFAULT if S is None else S
        f0, s0, _ = dec.split_stats()
        got = dec.decode(stream)
        assert np.array_equal(got, rgb), (S, int((got != rgb).sum()))
        f1, s1, _ = dec.split_stats()
        nsub = plan(n, size)[0]
        assert (f1 - f0, s1 - s0) == ((1, nsub) if nsub >= 2 else (0, 0)), (S, n)
        if n > 2 * size:
            assert f1 == f0 + 1 and s1 - s0 > 1


# the subsequences a frame is cut into, and the bytes asked for: the lane counts 64 .. 1024 at their edges
EDGES = [(2, 4096), (63, 16), (64, 16), (65, 16), (127, 16), (128, 16), (129, 16), (255, 8), (256, 8), (257, 8), (511, 8), (512, 8),
         (513, 8), (1023, 8), (1024, 8)]


def _noise_case(dec, stream, S, nsub):
    dec.split = S
    f0, s0, _ = dec.split_stats()
    got = dec.decode(stream)
    f1, s1, rounds = dec.split_stats()
    assert (f1 - f0, s1 - s0) == (1, nsub)                   # what the kernel itself counted
    assert 1 <= rounds <= 1024
    dec.split = 0
    plain = dec.decode(stream)
    assert dec.split_stats()[:2] == (f1, s1)
    assert np.array_equal(got, plain), int((got != plain).sum())
    want = ref.decode(stream, STD)
    assert np.array_equal(got, want), int((got != want).sum())


@pytest.mark.parametrize("nsub,S", EDGES)
def test_lane_count_edges(dec, nsub, S):
    stream = noise_frame(1000 + nsub, S * (nsub - 1), S * nsub)
    assert plan(entropy_len(stream), S) == (nsub, S)
    _noise_case(dec, stream, S, nsub)


def test_more_than_1024_subsequences_asked_for_raises_their_size(dec):
    stream = noise_frame(99, 8600, 8700)
    n = entropy_len(stream)
    nsub, sp = plan(n, 8)
    assert n > 8 * 1024 and sp == 9 and 512 < nsub <= 1024
    _noise_case(dec, stream, 8, nsub)


def test_one_call_holds_both_kinds_of_frame(pkg, dec):
    a, rgb_a, _ = ref.load_fixture("mjpeg_97x65_422_q30_opt")
    b, rgb_b, _ = ref.load_fixture("mjpeg_97x65_422_q75_rst3")
    c = synth.sparse_frame(97, 65, "2x1", 4242, ri=0)
    assert [pkg.mjpeg_probe(s)["segments"] for s in (a, b, c)] == [1, 21, 1]
    want_c = ref.decode(c, STD)
    for S in (8, 64, None):
        dec.split = S
        f0, s0, _ = dec.split_stats()
        img, intact, status = _batch(dec, [a, b, c], 97, 65, pad_row=7, pad_frame=29)
        assert intact and (status == 0).all(), status
        assert np.array_equal(img[0], rgb_a) and np.array_equal(img[1], rgb_b) and np.array_equal(img[2], want_c), S
        f1, s1, _ = dec.split_stats()
        size = DEFAULT if S is None else S
        assert f1 - f0 == 2 and s1 - s0 == plan(entropy_len(a), size)[0] + plan(entropy_len(c), size)[0]


@pytest.mark.parametrize("k", range(8))
def test_damaged_frame_between_two_good_ones(dec, k):
    stream, rgb, z = ref.load_fixture("mjpeg_33x17_422_q90_corrupt")
    bad = ref.corrupted(stream, int(z["corrupt_pos"][k]), int(z["corrupt_val"][k]))
    dec.split = 0
    _, _, plain = _batch(dec, [stream, bad, stream], 33, 17)
    try:
        want = ref.decode(bad, STD)
    except ValueError:
        want = None
    for S in (8, 37):
        dec.split = S
        img, intact, status = _batch(dec, [stream, bad, stream], 33, 17, pad_row=5, pad_frame=11)
        assert intact
        assert np.array_equal(status, plain) and status[0] == 0 and status[2] == 0, (S, status, plain)
        assert np.array_equal(img[0], rgb) and np.array_equal(img[2], rgb)
        if status[1] == 0 and want is not None and max(synth.extent(bad, STD)) <= synth.DOMAIN:
            assert np.array_equal(img[1], want), (S, int((img[1] != want).sum()))
    assert np.array_equal(dec.decode(stream), rgb)           # the handle is as good as new afterwards


def test_saturating_dc_walk(pkg):
    stream = saturating_dc_stream()
    d = pkg.HIPMJPEGDecoder(960, 8, max_stream_bytes=65536, split=0)
    plain = d.decode(stream)
    d.split = 8
    got = d.decode(stream)
    frames, nsub, rounds = d.split_stats()
    assert frames == 1 and nsub == plan(entropy_len(stream), 8)[0] >= 64 and 1 <= rounds <= nsub
    assert np.array_equal(got, plain), int((got != plain).sum())
    assert plain.min() == 0 and plain.max() == 255           # both ends of the walk show
    d.close()


def test_results_are_identical_run_to_run(dec):
    streams = [noise_frame(7, 3000, 3100), noise_frame(8, 5000, 5100), noise_frame(9, 700, 800)]
    dec.split = 8
    first, _, st = _batch(dec, streams, NOISE_W, NOISE_H)
    assert (st == 0).all()
    for _ in range(3):
        again, _, _ = _batch(dec, streams, NOISE_W, NOISE_H)
        assert np.array_equal(first, again)


def test_compute_mjpeg_on_a_pair_without_restart_intervals(pkg, dec):
    left = ref.load_fixture("mjpeg_97x65_422_q30_opt")[0]
    right = synth.sparse_frame(97, 65, "2x1", 4243, ri=0)
    W, H = 97, 65
    rng = np.random.default_rng(5)
    yy, xx = np.mgrid[0:H, 0:W]
    maps = []
    for _ in range(2):          # a mild warp: source = pixel + a sub-pixel offset, CV_16SC2 fixed point
        fxm = np.clip(xx + 1.5 + rng.random((H, W)), 0, W - 2)
        fym = np.clip(yy + 0.75 + rng.random((H, W)), 0, H - 2)
        ix, iy = np.floor(fxm).astype(np.int16), np.floor(fym).astype(np.int16)
        frac = (np.floor((fym - iy) * 32).astype(np.uint16) * 32 + np.floor((fxm - ix) * 32).astype(np.uint16))
        maps += [np.stack([ix, iy], -1), frac]
    roi = (8, 4, 80, 56)
    rc = pkg.HIPRectifier(maps[0], maps[1], maps[2], maps[3], roi)
    bm = pkg.HIPMatcher(numOfDisparities=16, blockSize=7, width=roi[2], height=roi[3], textureThreshold=0, uniquenessRatio=0,
                        speckleWindowSize=0, disp12MaxDiff=-1)
    dec.split = 0
    want = rc.compute(bm, dec.decode(left), dec.decode(right))
    assert np.array_equal(dec.compute(bm, rc, left, right), want)
    for S in (8, None):
        dec.split = S
        f0 = dec.split_stats()[0]
        got = dec.compute(bm, rc, left, right)
        assert dec.split_stats()[0] == f0 + 2
        assert np.array_equal(got, want), S
        assert np.array_equal(rc.compute(bm, dec.decode(left), dec.decode(right)), want)
