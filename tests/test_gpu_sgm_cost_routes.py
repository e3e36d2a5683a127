"""The rows of the StereoSGBM cost-route table ("SGM: cost routes") on the device, through the cases of
sgm_cost_routes.py: one pair through `compute` and three through `compute_device`, every frame bit for bit against the
reference that owns the case's form and mode (the oracle for gray Birchfield-Tomasi, sgm_cn_ref for colour and large ftzero,
sgm_census_ref for census, sgm_hh4_ref for MODE_HH4, sgm_3way_ref for MODE_SGBM_3WAY).  That each case plans to the route its
row names, and that its expected frames are live, different and not refused, is asserted without a device in
test_sgm_cost_plan_cpu.py."""
import numpy as np
import pytest

import sgm_cost_routes as routes
from conftest import load

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    import torch                         # torch first: it brings its own HIP runtime and must initialise before ours
    assert torch.cuda.is_available(), "the -m gpu suite needs an MI355X"
    return load()


@pytest.mark.parametrize("case", routes.CASES, ids=lambda c: c.name)
def test_cost_route(pkg, oracle, case):
    import torch
    c = case
    frames = c.frames()
    Ls, Rs = np.stack([f[0] for f in frames]), np.stack([f[1] for f in frames])
    want = [c.want(L, R, oracle) for L, R in frames]
    M = pkg.HIPSemiGlobalMatcher
    kw = dict(cost=M.COST_CENSUS, census=c.census) if c.census else {}
    pkg.binding.lib().rtdm_debug_sgm_cost16(c.f16)
    try:
        m = M(numOfDisparities=c.D, blockSize=c.bs, P1=routes.P1, P2=c.P2, width=c.W, height=c.H, max_batch=3, preFilterCap=c.cap,
              paths=5 if c.paths == 3 else c.paths, **kw)
        try:
            if c.paths == 3:
                m.setMode(M.MODE_SGBM_3WAY)
            one = m.compute(Ls[0], Rs[0])                                # (a refused frame raises)
            dD = torch.zeros((3, c.H, c.W), dtype=torch.int16, device="cuda")
            m.compute_device(torch.from_numpy(Ls).cuda(), torch.from_numpy(Rs).cuda(), dD, torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            three = dD.cpu().numpy()
            if c.paths == 3:
                assert m.path_variant == "vert3"
        finally:
            m.close()
    finally:
        pkg.binding.lib().rtdm_debug_sgm_cost16(0)
    assert one.tobytes() == want[0].tobytes(), "n = 1: %d pixels differ" % int((one != want[0]).sum())
    for i in range(3):
        assert three[i].tobytes() == want[i].tobytes(), "n = 3, frame %d: %d pixels differ" % (i, int((three[i] != want[i]).sum()))
    assert (want[0] != -16).any() and len({w.tobytes() for w in want}) == 3        # live frames, all different
