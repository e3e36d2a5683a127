"""tests/d3_walk_model.py proves its own sensitivity: on its scene the bits of a box's sums depend on the order of the additions,
so the two GPU tests that compare bits with it (test_the_walk_of_a_box_is_rule_d3 in tests/test_gpu_depth_objects.py and
tests/test_gpu_measure.py) cannot pass a kernel that adds row-major, folds its lanes another way or adds its bands in
descending order.  The thresholds are what the module's docstring reasons out, taken with a margin: about half of the 39 boxes
for row-major, a quarter for the fold, a quarter of the 10 boxes of three bands for the band order (at least one box for every
sum, two for the depth call's, six over the four sums)."""
import numpy as np
import pytest

import d3_walk_model as d3
import xyz_ref as xr

AT_LEAST = {"row_major": 12, "fold_neighbours": 6, "bands_descending": 1}     # boxes, for every one of the four sums


@pytest.mark.parametrize("labels", [False, True])
def test_another_order_changes_the_bits(labels):
    changed = d3.order_matters(labels)
    assert set(changed) == set(AT_LEAST)
    for order, (depth, xyz) in changed.items():
        assert min([depth] + xyz) >= AT_LEAST[order], (order, depth, xyz)
    depth, xyz = changed["bands_descending"]
    assert depth >= 2 and depth + sum(xyz) >= 6, (depth, xyz)                 # of 10 boxes with three bands, four sums each


def test_the_scene_is_what_the_gpu_tests_need():
    disp, mask, labels, boxes = d3.scene()
    assert len(boxes) == 39 == d3.CAP - 1 and {(b[2], b[3]) for b in boxes[:35]} == {(w, h) for w in d3.WIDTHS for h in d3.HEIGHTS}
    three_bands = [b for b in boxes if d3.lr.clipped(b, d3.W, d3.H)[3] > 2 * d3.BAND]
    assert len(three_bands) == 10
    assert sum(d3.lr.clipped(b, d3.W, d3.H) != b[:4] for b in boxes) >= 6                   # boxes that leave the frame
    assert (disp % 16 == 0).all() and 0.1 < (disp == d3.FILTERED).mean() < 0.2 and 0.2 < (mask == 0).mean() < 0.3
    # fused or not, ROUNDED or FIXED16: one Z, and the model's own statement of it is xyz_ref's
    z, counts = d3.depth_z(disp)
    for mode in (xr.ROUNDED, xr.FIXED16):
        assert np.array_equal(xr.reproject(disp, d3.Q, mode, True)[..., 2], z)
    assert float(np.abs(z[counts]).max()) < 1e4 and float(np.abs(z[counts]).min()) > 0 and 0.01 < (z[counts] > 9000).mean() < 0.04
    d = disp.astype(np.int64) // 16
    assert all(float(np.float64(k) + d3.C0) == float(k - 1000) + 2.0 ** -30 for k in np.unique(d))    # h_3 is exact
