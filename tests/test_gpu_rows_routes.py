"""A row of every kernel form of the left-right check and the speckle filter (plan_lrcheck / plan_speckle in k_rows.hip; the
table of DESIGN.md, "K3 / K4: routes", kept in tests/rows_cases.py) against the oracle, bit for bit and without an environment
hook: a single frame through compute, the batches of 129 through compute_device, first and last frame compared.
tests/test_rows_plan_cpu.py pins what is planned for each row.  Every compared frame is first shown, on the oracle alone, to
be live for the stages the row runs: the left-right check and the speckle filter each remove at least 5 pixels and at least
100 survive.  (The forms behind the hooks stay with test_gpu_round3.py, test_gpu_speckle_settled.py and
test_gpu_speckle_extruded.py.)"""
import functools

import numpy as np
import pytest

import rows_cases as RC
from conftest import load
from test_gpu_dslice import assert_same

pytestmark = pytest.mark.gpu

HOOKS = ("RTDM_LR_PAIRS", "RTDM_LR_PACKED", "RTDM_MERGE_REC_FUSED")
ROWS = RC.gpu_rows()


@pytest.fixture(scope="module")
def pkg():
    import torch                         # torch first: it brings its own HIP runtime and must initialise before ours
    assert torch.cuda.is_available(), "the -m gpu suite needs an MI355X"
    return load()


@functools.lru_cache(maxsize=None)
def _stream(synth, no):
    r = next(r for r in ROWS if r["no"] == no)
    L, R = RC.stream(synth, r)
    L.setflags(write=False); R.setflags(write=False)
    return L, R


@pytest.mark.parametrize("r", ROWS, ids=lambda r: "row%s-%dx%d-D%d-w%d-n%d" % (r["no"], r["W"], r["H"], r["D"], r["w"], r["n"]))
def test_row_matches_the_oracle(pkg, oracle, synth, monkeypatch, r):
    import torch
    for h in HOOKS:
        monkeypatch.delenv(h, raising=False)
    W, H, n = r["W"], r["H"], r["n"]
    L, R = _stream(synth, r["no"])
    want = {}
    for f in RC.frames(r):
        want[f], lr, spk, alive = RC.liveness(oracle, r, L[f], R[f])
        print(RC.assert_live(r, f, lr, spk, alive))
    m = pkg.HIPMatcher(numOfDisparities=r["D"], blockSize=r["w"], preFilterCap=r["cap"], disp12MaxDiff=r["maxdiff"],
                       speckleWindowSize=r["window"], speckleRange=32, width=W, height=H, max_batch=n)
    if n == 1:
        got = m.compute(L[0], R[0])[None]
    else:
        dL, dR = torch.from_numpy(np.array(L)).cuda(), torch.from_numpy(np.array(R)).cuda()
        dD = torch.empty((n, H, W), dtype=torch.int16, device="cuda")
        m.compute_device(dL, dR, dD, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        got = dD.cpu().numpy()
    m.close()
    for f in RC.frames(r):
        assert_same(got[f], want[f], "row %s frame %d" % (r["no"], f))
