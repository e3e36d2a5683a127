"""Every case of tests/lr_cases.py through HIPMatcher against the oracle, bit for bit and without an environment hook: the
left-right check's six kernel forms (five reachable), with and without the speckle filter's fused row init, on frames that
make every decision of the check live, hand it costs with their top bits set, sit on either side of every reachable bound of
the packed form's guard (two_ok_for_pk in k_rows.hip) and at both ends of int16.  tests/test_lr_states_cpu.py shows without a
device that the cases do what they claim and that a subtly wrong check would differ from the oracle on them;
tests/test_rows_plan_cpu.py pins the form each case is planned on.

One frame goes through compute, more through one compute_device call: up to four distinct frames, a longer batch repeats four
on the device (the first and the last are compared on the host, all of them on the device).  Output planes start as a sentinel.

The handle has no getter for the form its check ran on: that a case runs on the form it is named after rests on
tests/test_rows_plan_cpu.py, which plans every case with rows_aligned = true.  That is what the device path passes today --
compute, and compute_device with W % 8 != 0, run on the handle's own plane (rows of W rounded up to 8 elements in one aligned
allocation), and the contiguous int16 tensors handed to compute_device with W % 8 == 0 are 16-byte aligned in base, pitch and
frame stride.  A change to rows_aligned() or to bm_run_chunk's choice of plane has to be mirrored in that test's lr mode."""
import functools

import numpy as np
import pytest

import lr_cases as lc
from conftest import load
from test_gpu_dslice import assert_same

pytestmark = pytest.mark.gpu

HOOKS = ("RTDM_LR_PAIRS", "RTDM_LR_PACKED", "RTDM_MERGE_REC_FUSED")
SENTINEL = 12345


@pytest.fixture(scope="module")
def pkg():
    import torch                         # torch first: it brings its own HIP runtime and must initialise before ours
    assert torch.cuda.is_available(), "the -m gpu suite needs an MI355X"
    return load()


@functools.lru_cache(maxsize=None)
def _wants(oracle, cid):
    """the oracle's map of every source frame of the case, computed once"""
    c = next(c for c in lc.CASES if c["id"] == cid)
    L, R = lc.sources(c)
    want = np.stack([lc.want_map(oracle, c, L[s], R[s]) for s in range(L.shape[0])])
    want.setflags(write=False)
    return want


def matcher(pkg, c, n):
    m = pkg.HIPMatcher(numOfDisparities=c["D"], blockSize=c["w"], minDisparity=c["minD"], preFilterCap=c["cap"], textureThreshold=0,
                       uniquenessRatio=0, disp12MaxDiff=c["M"], speckleWindowSize=c["window"], speckleRange=c["range"], width=c["W"],
                       height=c["H"], max_batch=n)
    if c["roi"]:
        m.setROI1(c["roi"])
    return m


@pytest.mark.parametrize("c", lc.CASES, ids=lambda c: c["id"])
def test_case_matches_the_oracle(pkg, oracle, monkeypatch, c):
    import torch
    for h in HOOKS:
        monkeypatch.delenv(h, raising=False)
    W, H, n = c["W"], c["H"], c["n"]
    L, R = lc.sources(c)
    want = _wants(oracle, c["id"])
    src = lc.source_of(c)
    inv = (c["minD"] - 1) * 16
    m = matcher(pkg, c, n)
    try:
        if n == 1:
            got = m.compute(L[0], R[0], out=np.full((H, W), SENTINEL, np.int16))[None]
        else:
            idx = torch.from_numpy(src).cuda()
            dL, dR = torch.from_numpy(np.array(L)).cuda()[idx].contiguous(), torch.from_numpy(np.array(R)).cuda()[idx].contiguous()
            dD = torch.full((n, H, W), SENTINEL, dtype=torch.int16, device="cuda")
            m.compute_device(dL, dR, dD, torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            differ = (dD != torch.from_numpy(np.array(want)).cuda()[idx]).flatten(1).any(1).nonzero().flatten()
            got = dD.cpu().numpy()
    finally:
        m.close()
    for f in lc.compared(c):
        assert (want[src[f]] != inv).sum() >= (lc.ALIVE_THIN if c["thin"] else lc.ALIVE), c["id"]
        assert_same(got[f], want[src[f]], "%s frame %d" % (c["id"], f))
    if n > 1:
        assert differ.numel() == 0, "%s: %d frames differ, first %d" % (c["id"], differ.numel(), int(differ[0]))


@pytest.mark.parametrize("c", [c for c in lc.CASES if c["roi"]], ids=lambda c: c["id"])
def test_roi_from_device_memory_matches_the_oracle(pkg, oracle, monkeypatch, c):
    # the ROI1 of tests/test_gpu_bm_rois.py's kind: read on the device, the check runs under the envelope and without the init
    import torch
    for h in HOOKS:
        monkeypatch.delenv(h, raising=False)
    L, R = lc.sources(c)
    want = _wants(oracle, c["id"])
    m = matcher(pkg, dict(c, roi=None), 1)
    try:
        dD = torch.full((1, c["H"], c["W"]), SENTINEL, dtype=torch.int16, device="cuda")
        rois = torch.tensor([c["roi"]], dtype=torch.int32).cuda().contiguous()
        m.compute_device(torch.from_numpy(np.array(L)).cuda(), torch.from_numpy(np.array(R)).cuda(), dD, rois=rois)
        torch.cuda.synchronize()
        got = dD.cpu().numpy()
    finally:
        m.close()
    assert_same(got[0], want[0], "%s by rois=" % c["id"])
