"""The MJPEG decoder on the device (rtdm_mjpeg_*, k_mjpeg.hip) against the images Pillow / libjpeg-turbo decoded from the stored
streams: byte for byte, tolerance zero (rules J1-J5).  The damaged streams used here are the eight that
test_mjpeg_cpu.py has already run through the host build of the same decoding loop under the address sanitizer."""
import numpy as np
import pytest

import mjpeg_ref as ref
import mjpeg_synth as synth
from conftest import load

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    import torch                         # torch first: it brings its own HIP runtime and must initialise before ours
    assert torch.cuda.is_available()
    return load()


@pytest.fixture(scope="module")
def fx():
    return {n: ref.load_fixture(n)[:2] for n in ref.FIXTURES}


@pytest.fixture(scope="module")
def dec(pkg):
    d = pkg.HIPMJPEGDecoder(264, 96, max_batch=4, max_stream_bytes=8192)
    yield d
    d.close()


def _batch(pkg, dec, streams, W, H, pad_row=0, pad_frame=0, want_status=True):
    """decode_batch into a tensor whose rows and frames are padded and pre-filled with 0xA5 -> (frames, padding intact, status)"""
    import torch
    n, row = len(streams), W * 3 + pad_row
    flat = torch.full((n, H * row + pad_frame), 0xA5, dtype=torch.uint8, device="cuda")
    view = torch.as_strided(flat, (n, H, W, 3), (H * row + pad_frame, row, 3, 1))
    status = torch.full((n,), 77, dtype=torch.int32, device="cuda") if want_status else None
    dec.decode_batch(streams, out=view, status=status)
    torch.cuda.synchronize()
    host = flat.cpu().numpy()
    img = np.lib.stride_tricks.as_strided(host, (n, H, W, 3), (host.strides[0], row, 3, 1))
    mask = np.ones(host.shape, bool)
    np.lib.stride_tricks.as_strided(mask, (n, H, W * 3), (mask.strides[0], row, 1))[...] = False
    intact = bool((host[mask] == 0xA5).all())
    return img.copy(), intact, (status.cpu().numpy() if want_status else None)


@pytest.mark.parametrize("name", ref.FIXTURES)
def test_single_frame_equals_pillow(dec, fx, name):
    stream, rgb = fx[name]
    got = dec.decode(stream)
    assert got.shape == rgb.shape
    assert np.array_equal(got, rgb), "%d bytes differ" % int((got != rgb).sum())


def test_single_frame_honours_the_host_pitch_and_trailing_bytes(pkg, dec, fx):
    stream, rgb = fx["mjpeg_33x17_422_q90"]
    H, W = rgb.shape[:2]
    buf = np.full((H, W * 3 + 13), 0xA5, np.uint8)
    out = np.lib.stride_tricks.as_strided(buf, (H, W, 3), (buf.strides[0], 3, 1))
    dec.decode(stream + b"\x00\xff\xd9junk after EOI", out=out)          # len is a buffer size
    assert np.array_equal(out, rgb) and (buf[:, W * 3:] == 0xA5).all()


@pytest.mark.parametrize("name", ref.FIXTURES)
def test_batch_entry_with_padded_pitch_and_stride(pkg, dec, fx, name):
    stream, rgb = fx[name]
    H, W = rgb.shape[:2]
    img, intact, status = _batch(pkg, dec, [stream, stream, stream], W, H, pad_row=7, pad_frame=29)
    assert intact, "padding bytes were written"
    assert (status == 0).all()
    for k in range(3):
        assert np.array_equal(img[k], rgb), (k, int((img[k] != rgb).sum()))


def test_chunked_batch_equals_single_calls(pkg, fx):
    streams = [fx[n][0] for n in ref.BATCH]
    small = pkg.HIPMJPEGDecoder(97, 65, max_batch=2, max_stream_bytes=4096)
    img, intact, status = _batch(pkg, small, streams, 97, 65, pad_row=0, pad_frame=0)
    assert (status == 0).all()
    for k, n in enumerate(ref.BATCH):
        single = small.decode(streams[k])
        assert np.array_equal(single, fx[n][1])
        assert np.array_equal(img[k], single), k
    # without a status array, too
    img2, _, _ = _batch(pkg, small, streams, 97, 65, want_status=False)
    assert np.array_equal(img2, img)
    small.close()


def test_one_handle_serves_smaller_frames_in_turn(dec, fx):
    for name in ("mjpeg_33x17_422_q90", "mjpeg_97x65_422_q75_rst3", "mjpeg_16x8_422_q75", "mjpeg_33x17_422_q90"):
        assert np.array_equal(dec.decode(fx[name][0]), fx[name][1]), name


def test_frames_of_one_call_may_differ_in_tables(pkg, dec, fx):
    # 96x64 4:2:2: no DHT (standard tables) next to ordinary DHTs; 97x65 4:2:2: optimised tables and quality 30 next to
    # quality 75 with restart intervals
    for names in (("mjpeg_96x64_422_q75_nodht", "mjpeg_96x64_422_q75_gradient", "mjpeg_96x64_422_q75_nodht"),
                  ("mjpeg_97x65_422_q30_opt", "mjpeg_97x65_422_q75_rst3", "mjpeg_97x65_422_q75_batch2")):
        H, W = fx[names[0]][1].shape[:2]
        img, _, status = _batch(pkg, dec, [fx[n][0] for n in names], W, H)
        assert (status == 0).all()
        for k, n in enumerate(names):
            assert np.array_equal(img[k], fx[n][1]), n


def test_refusals_reach_no_frame_of_the_call(pkg, dec, fx):
    B = pkg.binding
    a, b = fx["mjpeg_96x64_422_q75_nodht"][0], fx["mjpeg_97x65_422_q75_rst3"][0]
    with pytest.raises(B.RtdmError) as e:
        _batch(pkg, dec, [a, b], 96, 64)                     # sizes differ
    assert e.value.status == -2
    with pytest.raises(B.RtdmError) as e:
        _batch(pkg, dec, [a, a[:-2]], 96, 64)                # no EOI
    assert e.value.status == -8
    out = np.empty((64, 96, 3), np.uint8)
    assert B.lib().rtdm_mjpeg_decode(dec._h, a, len(a), 96, 48, out.ctypes.data, 96 * 3) == -2
    big = pkg.HIPMJPEGDecoder(64, 64)
    assert B.lib().rtdm_mjpeg_decode(big._h, a, len(a), 96, 64, out.ctypes.data, 96 * 3) == -2       # larger than the handle
    big.close()


@pytest.mark.parametrize("k", range(8))
def test_damaged_frame_between_two_good_ones(pkg, dec, k):
    stream, rgb, z = ref.load_fixture("mjpeg_33x17_422_q90_corrupt")
    bad = ref.corrupted(stream, int(z["corrupt_pos"][k]), int(z["corrupt_val"][k]))
    assert pkg.mjpeg_probe(bad)["segments"] == 1             # the host parser lets it through: the kernel meets the damage
    img, intact, status = _batch(pkg, dec, [stream, bad, stream], 33, 17, pad_row=5, pad_frame=11)      # the call returns
    assert intact
    assert np.array_equal(img[0], rgb) and np.array_equal(img[2], rgb)
    assert status[0] == 0 and status[2] == 0 and status[1] in (0, -8)
    # the single-frame entry reports the same verdict, and the handle is as good as new afterwards
    out = np.empty_like(rgb)
    st = pkg.binding.lib().rtdm_mjpeg_decode(dec._h, bad, len(bad), 33, 17, out.ctypes.data, 33 * 3)
    assert st == int(status[1])
    assert np.array_equal(dec.decode(stream), rgb)
    # damage that still decodes, and stays inside the domain the rules are pinned on (mjpeg_synth.py), gives the image the rules
    # give; test_stored_corruptions_that_decode_stay_in_the_domain has checked on the host build that this is reached
    try:
        want = ref.decode(bad, ref.std_tables())
    except ValueError:
        want = None
    if status[1] == 0 and want is not None and max(synth.extent(bad, ref.std_tables())) <= synth.DOMAIN:
        assert np.array_equal(img[1], want), int((img[1] != want).sum())
        assert np.array_equal(out, want)


def test_compute_mjpeg_equals_decode_then_compute_rgb(pkg, dec, fx):
    names = ("mjpeg_97x65_422_q75_batch0", "mjpeg_97x65_422_q75_batch1")
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
    # no filtering: every searched pixel keeps a disparity, so the map depends on which frame is the left one
    bm = pkg.HIPMatcher(numOfDisparities=16, blockSize=7, width=roi[2], height=roi[3], textureThreshold=0, uniquenessRatio=0,
                        speckleWindowSize=0, disp12MaxDiff=-1)
    got = dec.compute(bm, rc, fx[names[0]][0], fx[names[1]][0])
    want = rc.compute(bm, dec.decode(fx[names[0]][0]), dec.decode(fx[names[1]][0]))
    assert np.array_equal(got, want)
    assert (want != bm.filtered).mean() > 0.3
    assert not np.array_equal(dec.compute(bm, rc, fx[names[1]][0], fx[names[0]][0]), got)
    assert np.array_equal(dec.compute(bm, rc, fx[names[0]][0], fx[names[1]][0]), got)        # run to run


def test_results_are_identical_run_to_run(pkg, dec, fx):
    streams = [fx[n][0] for n in ref.BATCH[:4]]
    first, _, _ = _batch(pkg, dec, streams, 97, 65)
    for _ in range(3):
        again, _, _ = _batch(pkg, dec, streams, 97, 65)
        assert np.array_equal(first, again)
