"""The speckle filter on extruded pairs (tests/extruded.py): every pixel in vertical contact with the one above it, thousands
of one-column components, long runs sitting on thin columns.  This is what reaches the filter's bookkeeping through the
public API: the overflow branch of the 1024-entry union queue, marks that travel dozens of rows, every count of checked
rows modulo the four-row blocks, every merge form.  Device and oracle are compared bit for bit; every case first asserts
on the oracle's UNFILTERED map that the input does ask that of the filter (tests/test_extruded_cpu.py asserts the same
without a GPU)."""
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

import extruded as E
from conftest import load, ROOT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    import torch
    assert torch.cuda.is_available(), "the -m gpu suite needs an MI355X"
    return load()


def assert_same(got, want, what):
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError("%s: %d / %d pixels differ; rows %d..%d; first at (y,x)=%s got %d want %d" % (
            what, len(bad), got.size, bad[:, 0].min(), bad[:, 0].max(), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])]))


# One string, run in a child process per setting (the hooks are read once per process).  Cases 1 - 4: every job of
# extruded.single_frame_jobs at every one of its windows.  Case 5: device-resident batches of four distinct pairs, cycled.
# The batch sizes pick the strip length of plan_speckle (k_rows.hip; rows x352 and x208 of tests/rows_cases.py pin it and
# carry the arithmetic): at 640 x 40, blockSize 9, 352 frames run k_spk_merge_strip<4, true> and 208 frames k_spk_merge_strip<2, true>
# (both under RTDM_LR_PAIRS=1; two pairs per workgroup leave the rec form + k_spk_merge_strip<1, true, true> at any batch size).
_CASES = r'''
import importlib, sys, zlib, numpy as np, torch
sys.path.insert(0, %r); sys.path.insert(0, %r)
pkg = importlib.import_module("rt-depth-map_amd")
from oracle import oracle as orc
import extruded as E
orc.build()

def hip_kw(kw):
    kw = dict(kw); kw["numOfDisparities"] = kw.pop("numDisparities"); kw.pop("roi1", None)
    return kw

def same(got, want, what):
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError((what, "pixels", len(bad), "rows", int(bad[:, 0].min()), int(bad[:, 0].max()), "first", tuple(int(v) for v in bad[0])))

ncmp = 0
for j in E.single_frame_jobs(orc):            # asserts each input's conditions on the oracle's unfiltered map first
    H, W = j["L"].shape
    for win in j["windows"]:
        kw = dict(j["kw"], speckleWindowSize=win)
        want = orc.bm_compute(j["L"], j["R"], nthreads=8, **kw)
        m = pkg.HIPMatcher(width=W, height=H, **hip_kw(kw))
        if kw.get("roi1"): m.setROI1(kw["roi1"])
        got = m.compute(j["L"], j["R"])
        m.close()
        same(got, want, (j["name"], win))
        if win >= j["hv"] or "marks" in j["name"]:
            assert (want != j["d"]).any(), (j["name"], win, "the filter removed nothing")
        ncmp += 1
        print("CRC", j["name"], win, zlib.crc32(got.tobytes()))

jobs = list(E.batch_jobs(orc))
hv = jobs[0]["hv"]
assert all(j["hv"] == hv for j in jobs)
kw = dict(jobs[0]["kw"], speckleWindowSize=hv)
want = [orc.bm_compute(j["L"], j["R"], nthreads=8, **kw) for j in jobs]
assert len({w.tobytes() for w in want}) == 4
for n in (352, 208):
    idx = np.arange(n) %% 4
    Ls = np.stack([jobs[i]["L"] for i in range(4)])[idx]; Rs = np.stack([jobs[i]["R"] for i in range(4)])[idx]
    m = pkg.HIPMatcher(width=640, height=40, max_batch=n, **hip_kw(kw))
    dL, dR = torch.from_numpy(Ls).cuda(), torch.from_numpy(Rs).cuda()
    dD = torch.empty((n, 40, 640), dtype=torch.int16, device="cuda")
    m.compute_device(dL, dR, dD, torch.cuda.current_stream().cuda_stream); torch.cuda.synchronize()
    got = dD.cpu().numpy()
    m.close()
    for i in list(range(4)) + list(range(n - 4, n)):
        same(got[i], want[i %% 4], ("batch", n, i))
        ncmp += 1
    print("CRC", "batch", n, zlib.crc32(got.tobytes()))
print("compared", ncmp)
print("ok")
'''
N_SINGLE = 2 * 4 + 5 + 14 + (3 * 2 + 1)          # (job, window) comparisons of cases 1 - 4
N_CRC = N_SINGLE + 2

SETTINGS = (("auto", {}), ("pairs1", {"RTDM_LR_PAIRS": "1"}), ("pairs2", {"RTDM_LR_PAIRS": "2"}),
            ("vec1", {"RTDM_LR_PAIRS": "1", "RTDM_LR_PACKED": "0"}), ("rec_unfused", {"RTDM_MERGE_REC_FUSED": "0"}))


def test_every_merge_form_matches_the_oracle_on_extruded_pairs():
    base = {k: v for k, v in os.environ.items() if k not in ("RTDM_LR_PAIRS", "RTDM_LR_PACKED", "RTDM_MERGE_REC_FUSED")}
    outs = {}
    for name, extra in SETTINGS:            # one at a time; the first child that does not end cleanly ends the test
        p = subprocess.run([sys.executable, "-c", _CASES % (ROOT, os.path.join(ROOT, "tests"))], stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, text=True, timeout=300, env=dict(base, **extra))
        assert p.returncode == 0 and p.stdout.strip().endswith("ok"), (name, p.returncode, p.stdout[-400:], p.stderr[-3000:])
        outs[name] = [ln for ln in p.stdout.splitlines() if ln.startswith("CRC")]
        assert len(outs[name]) == N_CRC and "compared %d" % (N_SINGLE + 16) in p.stdout, (name, len(outs[name]))
    assert all(v == outs["auto"] for v in outs.values()), [k for k, v in outs.items() if v != outs["auto"]]


def test_a_frame_wider_than_4096_is_refused(pkg):
    # both matchers keep whole rows in LDS and refuse such frames at creation, so no extruded input reaches the wide-frame
    # selections of plan_lrcheck; the scalar k_lrcheck is reached by SAD sums past 16 bits instead (extruded.head_jobs)
    B = load("binding")
    with pytest.raises(B.RtdmError):
        pkg.HIPMatcher(numOfDisparities=16, blockSize=9, width=4104, height=24)
    with pytest.raises(B.RtdmError):
        pkg.HIPSemiGlobalMatcher(numOfDisparities=16, width=4104, height=24)


# ---- cv::StereoSGBM: sgm_finish hands the filter per-pixel heads; 640 wide runs k_spk_merge_strip<4, false> (whose threads walk
# four row pairs: a workgroup meets ~2900 contacts, the queue overflows), 644 wide k_spk_merge (no queue) -------------------------
@pytest.fixture(scope="module")
def sgm_unfiltered(oracle):
    return {(W, paths, r): oracle.sgm_compute(E.sgm_frames(W)[0], E.sgm_frames(W)[1], speckleWindowSize=0, speckleRange=r,
                                              paths=paths, **E.SGM)
            for W in (640, 644) for paths in (8, 5) for r in (0, 1)}


@pytest.mark.parametrize("W,paths,rng_,win", E.SGM_CASES)
def test_sgm_three_bands(pkg, oracle, sgm_unfiltered, W, paths, rng_, win):
    L, R = E.sgm_frames(W)
    d = sgm_unfiltered[(W, paths, rng_)]
    if rng_ == 0:
        n, depth = E.require_rescue(d, -16, 0, win)
        cand = E.new_run_contacts(d, -16, 0)
        if W % 8 == 0:
            assert E.max_contacts_per_workgroup(cand, range(1, 88), 4) >= E.OVERFLOW_MIN
    want = oracle.sgm_compute(L, R, speckleWindowSize=win, speckleRange=rng_, paths=paths, **E.SGM)
    kw = dict(E.SGM); kw["numOfDisparities"] = kw.pop("numDisparities")
    m = pkg.HIPSemiGlobalMatcher(width=W, height=88, paths=paths, speckleWindowSize=win, speckleRange=rng_, **kw)
    got = m.compute(L, R)
    m.close()
    assert_same(got, want, ("sgm", W, paths, rng_, win))
    if rng_ == 0:
        assert (want != d).sum() >= 100            # the filter did remove the small components


def test_sgm_one_band_at_the_height_of_its_columns(pkg, oracle):
    L, R = E.sgm_frames(640, one_band=True)
    d = oracle.sgm_compute(L, R, speckleWindowSize=0, speckleRange=0, paths=8, **E.SGM)
    hv = E.band_height(d, -16, 0, 40)
    E.require_hv_boundary(oracle, d, -16, 0, hv)
    kw = dict(E.SGM); kw["numOfDisparities"] = kw.pop("numDisparities")
    for win in (hv - 1, hv):
        want = oracle.sgm_compute(L, R, speckleWindowSize=win, speckleRange=0, paths=8, **E.SGM)
        m = pkg.HIPSemiGlobalMatcher(width=640, height=40, paths=8, speckleWindowSize=win, speckleRange=0, **kw)
        got = m.compute(L, R)
        m.close()
        assert_same(got, want, ("sgm one band", win))


def test_marks_do_not_depend_on_scheduling(pkg, oracle):
    # five runs on one handle schedule the merge workgroups differently; which runs are marked first must not matter
    j = next(E.mark_jobs(oracle))
    assert j["name"] == "marks_r0_w3" and j["measured"]["rescue"][1] >= E.DEPTH_MIN
    kw = dict(j["kw"], speckleWindowSize=3); kw["numOfDisparities"] = kw.pop("numDisparities")
    want = oracle.bm_compute(j["L"], j["R"], nthreads=8, **dict(j["kw"], speckleWindowSize=3))
    m = pkg.HIPMatcher(width=640, height=88, **kw)
    crcs = []
    for i in range(5):
        got = m.compute(j["L"], j["R"])
        assert_same(got, want, ("run", i))
        crcs.append(zlib.crc32(got.tobytes()))
    m.close()
    assert len(set(crcs)) == 1
