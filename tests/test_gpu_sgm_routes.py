"""The rows of the StereoSGBM route table ("SGM: routes") that a handle reaches without a test hook, on the device:
one pair through `compute` and three through `compute_device`, every frame bit for bit against the oracle (MODE_HH4:
sgm_hh4_ref, the tests' reference of that mode), and the path variant and the number of row-synchronous sweeps that the row
says.  What plan_sgm plans for these rows, pass by pass, is pinned without a device in test_sgm_plan_cpu.py; the hooked rows
run in the child processes of test_gpu_round3.py and test_gpu_sgm_hh4.py."""
import numpy as np
import pytest

import sgm_hh4_ref
from conftest import load

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    import torch                         # torch first: it brings its own HIP runtime and must initialise before ours
    assert torch.cuda.is_available(), "the -m gpu suite needs an MI355X"
    return load()


def shifted_pair(seed, W, H, shift):
    """A textured pair whose right view is the left one moved by `shift` columns: L[x] = R[x - shift]."""
    rng = np.random.default_rng(seed)
    T = rng.integers(0, 256, (H, W + shift)).astype(np.float64)
    T = (T + np.roll(T, 1, 1) + np.roll(T, -1, 1) + np.roll(T, 1, 0) + np.roll(T, -1, 0)) / 5
    T = T.astype(np.uint8)
    return T[:, :W].copy(), T[:, shift:shift + W].copy()


# (row of the table, paths, D, W - D, H, variant, sweeps per call)
ROWS = [
    (1, 8, 64, 61, 23, "sweep", 2),
    (1, 8, 128, 61, 23, "sweep", 2),
    (2, 5, 96, 44, 18, "sweep", 1),
    (3, 4, 96, 44, 18, "vert", 0),
    (25, 8, 272, 20, 12, "wide_w1", 0),
    (26, 5, 1040, 20, 12, "wide_w4", 0),
]


@pytest.mark.parametrize("row,paths,D,W1,H,variant,sweeps", ROWS, ids=["row%d_D%d" % (r[0], r[2]) for r in ROWS])
def test_route(pkg, oracle, row, paths, D, W1, H, variant, sweeps):
    import torch
    W = D + W1
    frames = [shifted_pair(9100 + 13 * i + D + paths, W, H, 2 + 3 * i) for i in range(3)]
    Ls, Rs = np.stack([f[0] for f in frames]), np.stack([f[1] for f in frames])
    if paths == 4:
        want = [sgm_hh4_ref.sgm_compute(L, R, numDisparities=D, blockSize=5) for L, R in frames]
    else:
        want = [oracle.sgm_compute(L, R, numDisparities=D, blockSize=5, paths=paths) for L, R in frames]
    m = pkg.HIPSemiGlobalMatcher(numOfDisparities=D, blockSize=5, width=W, height=H, max_batch=3, paths=paths)
    try:
        one = m.compute(Ls[0], Rs[0])
        assert (m.path_variant, m.pass_stats()) == (variant, (sweeps, False))
        dD = torch.zeros((3, H, W), dtype=torch.int16, device="cuda")
        m.compute_device(torch.from_numpy(Ls).cuda(), torch.from_numpy(Rs).cuda(), dD, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        three = dD.cpu().numpy()
        assert (m.path_variant, m.pass_stats()) == (variant, (2 * sweeps, False))
    finally:
        m.close()
    assert one.tobytes() == want[0].tobytes(), "n = 1: %d pixels differ" % int((one != want[0]).sum())
    for i in range(3):
        assert three[i].tobytes() == want[i].tobytes(), "n = 3, frame %d: %d pixels differ" % (i, int((three[i] != want[i]).sum()))
    assert (want[0] != -16).any() and len({w.tobytes() for w in want}) == 3        # live frames, all different
