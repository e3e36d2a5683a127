"""The host entry points that stage pitched rows through rtdm::copy_rows (csrc/rtdm_rows.h; DESIGN.md, the table of host entry
points), on 157x113, 157x257 and 160x113 frames at D = 32, blockSize 9: 157 columns give internal rows of 160, 113 rows take
one band of the staged upload, 257 rows both bands with an odd split, and 160x113 with dense pitches the one-copy branches.

tests/host_staging_calls.py makes every call twice -- on dense arrays, and on views that start at column > 0 of parents with odd
pitches which END with the view's last row and hold 0xA5 around it -- and once in its device form on frames uploaded by torch.
Asserted: both layouts give identical outputs, the bytes around the views are untouched (Buf.take), every map has more than 5 %
non-FILTERED pixels, and the outputs equal the device forms' bit for bit.  rtdm_estimate_frame and rtdm_estimate_frame_classes
have no device form: their outputs are held to profiles/host_staging_hashes.txt, the listing taken on the parent of the change
that introduced copy_rows (and equal on that change)."""
import os

import numpy as np
import pytest

import host_staging_calls as hs
from conftest import ROOT

pytestmark = pytest.mark.gpu

FILTERED = -16                                   # (minDisparity - 1) * 16
LAYOUTS = ("dense", "view")


@pytest.fixture(scope="module")
def pkg():
    import torch                         # torch first: it brings its own HIP runtime and must initialise before ours
    assert torch.cuda.is_available()
    from conftest import load
    return load()


@pytest.fixture(scope="module")
def listing():
    lines = [ln.split() for ln in open(os.path.join(ROOT, "profiles", "host_staging_hashes.txt")) if ln[:1].isdigit()]
    return {(size, layout, name): digest for size, layout, name, digest in lines}


@pytest.fixture(scope="module", params=hs.SIZES, ids=lambda s: "%dx%d" % s)
def world(pkg, request):
    W, H = request.param
    rig = hs.Rig(pkg, W, H)
    w = dict(W=W, H=H, dense=hs.run_host(rig, False), view=hs.run_host(rig, True), device=hs.run_device(rig))
    rig.close()
    return w


def test_dense_arrays_and_padded_views_give_the_same(world):
    assert sorted(world["dense"]) == sorted(world["view"])
    for name, a in world["dense"].items():
        b = world["view"][name]
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), name


def test_every_map_is_mostly_matched(world):
    maps = [n for n in world["dense"] if n.endswith(".disp")]
    assert len(maps) == 8
    for name in maps:
        assert (world["dense"][name] != FILTERED).mean() > 0.05, name
    assert len(world["dense"]["objects_detect.boxes"]) >= 1 and len(world["dense"]["estimate_frame.boxes"]) >= 1
    assert (world["dense"]["estimate_batch.counts"].sum(1) >= 2).all()
    assert world["dense"]["estimate_frame.counts"].sum() > 0 and world["dense"]["bm_compute_depth.counts"].sum() > 0


@pytest.mark.parametrize("layout", LAYOUTS)
def test_outputs_are_the_device_forms(world, layout):
    host, dev = world[layout], world["device"]
    for name, want in dev.items():
        got = host[name]
        if name == "objects_detect.boxes":
            assert sorted(map(tuple, got.tolist())) == want
        else:
            assert got.shape == want.shape and got.tobytes() == want.tobytes(), name
    # the matcher's other host forms: the same map as rtdm_bm_compute_device's
    for name in ("bm_compute_page_locked.disp", "bm_compute_depth.disp"):
        assert host[name].tobytes() == dev["bm_compute.disp"].tobytes(), name
    for name in ("mean", "counts"):
        assert host["bm_compute_depth." + name].tobytes() == host["bm_compute_depth_no_disp." + name].tobytes()
    # without disp and measurements the batch call returns the same lists
    for name in ("objects", "counts", "mean", "npix"):
        assert host["estimate_batch." + name].tobytes() == host["estimate_batch_measured." + name].tobytes(), name


@pytest.mark.parametrize("layout", LAYOUTS)
def test_single_frame_estimates_are_the_recorded_ones(world, listing, layout):
    size = "%dx%d" % (world["W"], world["H"])
    names = [n for n in world[layout] if n.startswith("estimate_frame")]
    assert len(names) == 8
    for name in names:
        assert hs.sha(world[layout][name]) == listing[(size, layout, name)], name
