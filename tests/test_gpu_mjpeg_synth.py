"""The MJPEG decoder on the device against mjpeg_ref.decode on synthetic streams (mjpeg_synth.py), byte for byte.  Every stream
used here is held, in test_mjpeg_synth_cpu.py, against Pillow / libjpeg-turbo (which pins mjpeg_ref on it), against the host
build of the device's segment loop and against that build under the address and undefined-behaviour sanitizers; Pillow is not
needed here.  What the stored fixtures do not reach: k_mjpeg_huff with 128 and 256 lanes and with more segments than lanes,
k_mjpeg_idct with more than one workgroup and component boundaries at 255 / 256 / 257, every run/size symbol and code lengths
up to 16, table ids 2 and 3, restart structures, and J3 / J4 / the crop at every small size."""
import numpy as np
import pytest

import mjpeg_ref as ref
import mjpeg_synth as synth
from conftest import load
from test_gpu_mjpeg import _batch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    import torch                         # torch first: it brings its own HIP runtime and must initialise before ours
    assert torch.cuda.is_available()
    return load()


@pytest.fixture(scope="module")
def std():
    return ref.std_tables()


@pytest.fixture(scope="module")
def wide(pkg):
    """serves every frame of this module: up to 2056 x 136, 771 blocks, 520 segments"""
    d = pkg.HIPMJPEGDecoder(2056, 136, max_batch=8, max_stream_bytes=16384)
    yield d
    d.close()


def _same_shape_groups(items, std):
    groups = {}
    for label, s in items:
        f = ref.parse(s, std)
        groups.setdefault((f.W, f.H, f.ncomp, f.hs, f.vs), []).append((label, s))
    return groups


def _check_in_batches(pkg, dec, items, std, per_call=8):
    """frames of one size and sampling go through one batch call (at most per_call each); every image equals mjpeg_ref's"""
    for (W, H, _, _, _), group in _same_shape_groups(items, std).items():
        for i in range(0, len(group), per_call):
            part = group[i:i + per_call]
            img, intact, status = _batch(pkg, dec, [s for _, s in part], W, H, pad_row=5, pad_frame=3)
            assert intact, "padding bytes were written"
            for k, (label, s) in enumerate(part):
                assert max(synth.extent(s, std)) <= synth.DOMAIN, label
                want = ref.decode(s, std)
                assert status[k] == 0, label
                assert np.array_equal(img[k], want), (label, int((img[k] != want).sum()))


# ---- launch shapes ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def launch():
    return dict(synth.launch_frames())


@pytest.mark.parametrize("label", [k for k in synth.LAUNCH if not k.startswith("mix")])
def test_launch_shape(pkg, wide, std, launch, label):
    """single-frame calls: the frame's own segment count chooses 64, 128 or 256 lanes (test_launch_shapes_are_what_they_claim
    has the counts); the frames of 257 and more segments send lanes on a second and third trip; 257 and more blocks need a second,
    third and fourth workgroup of k_mjpeg_idct, and Cb starts at block 255, 256 and 257"""
    s = launch[label]
    assert max(synth.extent(s, std)) <= synth.DOMAIN
    want = ref.decode(s, std)
    got = wide.decode(s)
    assert np.array_equal(got, want), int((got != want).sum())
    _check_in_batches(pkg, wide, [(label, s), (label, s)], std)


def test_lanes_follow_the_largest_frame_of_the_call(pkg, wide, std, launch):
    a, b = launch["mix_1seg"], launch["mix_300seg"]
    for order in ((a, b), (b, a), (a, b, a)):
        img, intact, status = _batch(pkg, wide, list(order), 200, 96, pad_row=1, pad_frame=2)
        assert intact and (status == 0).all()
        for k, s in enumerate(order):
            assert np.array_equal(img[k], ref.decode(s, std)), k


# ---- the stream classes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["a", "b", "c", "d", "e"])
def test_stream_class(pkg, wide, std, name):
    _check_in_batches(pkg, wide, synth.class_streams(name), std)


# ---- J3 / J4 / the crop at every small size ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampling", ["2x1", "2x2", "1x1", "gray"])
def test_size_sweep(wide, std, sampling):
    bad = []
    for smp, W, H in synth.sweep_cases():
        if smp != sampling:
            continue
        s = synth.sweep_stream(smp, W, H)
        assert max(synth.extent(s, std)) <= synth.DOMAIN
        got, want = wide.decode(s), ref.decode(s, std)
        if got.shape != want.shape or not np.array_equal(got, want):
            bad.append((W, H))
    assert not bad, bad


# ---- batch plumbing -------------------------------------------------------------------------------------------------------------
def test_chunked_calls_with_every_stream_length_mod_16(pkg, std):
    frames = synth.residue_frames()
    dec = pkg.HIPMJPEGDecoder(40, 24, max_batch=3, max_stream_bytes=4096)
    singles = [dec.decode(s) for _, s in frames]
    for (label, s), img in zip(frames, singles):
        assert np.array_equal(img, ref.decode(s, std)), label
    for half in (frames[:8], frames[8:]):                    # 8 frames through a handle of 3: chunks of 3, 3 and 2
        img, intact, status = _batch(pkg, dec, [s for _, s in half], 40, 24, pad_row=7, pad_frame=29)
        assert intact and (status == 0).all()
        for k, (label, s) in enumerate(half):
            assert np.array_equal(img[k], ref.decode(s, std)), label
    # a frame of another size at position 5 of 8: the call is refused, and the handle decodes as before
    other = synth.sparse_frame(32, 24, "2x1", 800, ri=2)
    mixed = [s for _, s in frames[:8]]
    mixed[5] = other
    with pytest.raises(pkg.binding.RtdmError) as e:
        _batch(pkg, dec, mixed, 40, 24)
    assert e.value.status == -2
    img, _, status = _batch(pkg, dec, [s for _, s in frames[:8]], 40, 24)
    assert (status == 0).all()
    for k in range(8):
        assert np.array_equal(img[k], singles[k]), k
    assert np.array_equal(dec.decode(other), ref.decode(other, std))
    dec.close()
