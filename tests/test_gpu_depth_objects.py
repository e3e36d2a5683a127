"""rtdm_depth_objects_device alone (rules D1-D6 of DESIGN.md section 4.16): hand-made rtdm_object lists, random x16 maps with a
share of FILTERED pixels and random masks.  The expectation is oracle.depth_stats per object over its clipped box and its own
class plane, as tests/objects_batch_ref.depth does it.  Counts are exact; means are held to rtol 1e-9, the bound
tests/test_gpu_objects_batch.py holds this reduction to against the oracle's row-major order (for <= 4e5 same-sign terms
reordering a double sum moves it by about 4e-11 relative).  Q is the 320x240 calibration's, so no Z sits near the 1e4 threshold."""
import numpy as np
import pytest

import d3_walk_model as d3
import rectify_util as ru

pytestmark = pytest.mark.gpu

N, K, W, H, CAP = 3, 2, 300, 9, 80
FILTERED = -16                                   # (minDisparity - 1) * 16 of a matcher with minDisparity 0
MEAN0, NPIX0, OBJ0 = -777.0, -777, 0xA5          # what the outputs and the unused list entries hold before a call
Q = ru.calib("320x240")["Q"]


@pytest.fixture(scope="module")
def pkg():
    import torch                         # torch first: it brings its own HIP runtime and must initialise before ours
    assert torch.cuda.is_available()
    from conftest import load
    return load()


def frames(seed, n=N, w=W, h=H, filtered=0.2):
    """n random x16 maps (d in 2 .. 40 with every sixteenth, `filtered` of the pixels FILTERED) and n x K random masks."""
    rng = np.random.default_rng(seed)
    disp = rng.integers(32, 640, (n, h, w)).astype(np.int16)
    disp[rng.random((n, h, w)) < filtered] = FILTERED
    masks = rng.choice(np.array([0, 255, 255, 255, 1, 128], np.uint8), (n, K, h, w))
    return disp, masks


def clip(o, w=W, h=H):
    x, y, bw, bh, c = o
    x0, y0, x1, y1 = max(x, 0), max(y, 0), min(x + bw, w), min(y + bh, h)
    if bw <= 0 or bh <= 0 or x1 <= x0 or y1 <= y0 or not 0 <= c < K:
        return None
    return (x0, y0, x1 - x0, y1 - y0)


def expect(oracle, disp, masks, lists, counts, cap):
    """D1-D4 on the CPU -> (mean n x cap, npix n x cap) with the sentinels where nothing may be written."""
    n = len(lists)
    mean, npix = np.full((n, cap), MEAN0), np.full((n, cap), NPIX0, np.int32)
    for f in range(n):
        stored = min(int(np.maximum(counts[f], 0).sum()), cap)
        assert stored <= len(lists[f])
        mean[f, :stored], npix[f, :stored] = 0.0, 0
        for c in range(K):
            idx = [i for i in range(stored) if lists[f][i][4] == c and clip(lists[f][i], disp.shape[2], disp.shape[1])]
            if idx:
                m, k = oracle.depth_stats(disp[f], Q, masks[f, c], [clip(lists[f][i], disp.shape[2], disp.shape[1]) for i in idx])
                mean[f, idx], npix[f, idx] = m, k
    return mean, npix


def run(pkg, disp, masks, lists, counts, cap, padded=False, two=False, labels=False, q=Q):
    """One call (two: the same call twice on fresh outputs; labels: `masks` are int32 label planes and the call is the labels
    form) -> (mean n x cap, npix n x cap) on the host."""
    import torch
    n, h, w = disp.shape
    obj = np.full((n, cap * 32), OBJ0, np.uint8)
    rec = obj.view(pkg.OBJECT_DTYPE).reshape(n, cap)
    for f, lst in enumerate(lists):
        for i, o in enumerate(lst[:cap]):
            rec[f, i] = (o[0], o[1], o[2], o[3], o[4], 0, (0, 0))
    if padded:                                    # rows, frames and planes with padding that would wreck the result if read
        dbuf = torch.full((n, h + 1, w + 7), -32768, dtype=torch.int16, device="cuda")
        mbuf = torch.full((n, K, h + 2, w + 5), 255, dtype=torch.uint8, device="cuda")
        d_disp, d_masks = dbuf[:, :h, :w], mbuf[:, :, :h, :w]
        d_disp.copy_(torch.from_numpy(disp).cuda()); d_masks.copy_(torch.from_numpy(masks).cuda())
    else:
        d_disp, d_masks = torch.from_numpy(disp).cuda(), torch.from_numpy(masks).cuda()
    d_obj = torch.from_numpy(obj).cuda()
    d_cnt = torch.from_numpy(np.ascontiguousarray(counts, np.int32)).cuda()
    out = []
    for _ in range(2 if two else 1):
        d_mean = torch.full((n, cap), MEAN0, dtype=torch.float64, device="cuda")
        d_npix = torch.full((n, cap), NPIX0, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        fn = pkg.depth_objects_labels_device if labels else pkg.depth_objects_device
        ws = fn(d_disp, q, d_masks, d_obj, d_cnt, d_mean, d_npix, capacity=cap)
        torch.cuda.synchronize()
        del ws
        out.append((d_mean.cpu().numpy(), d_npix.cpu().numpy()))
    return out if two else out[0]


def check(got, want):
    assert np.array_equal(got[1], want[1]), np.argwhere(got[1] != want[1])[:8]
    np.testing.assert_allclose(got[0], want[0], rtol=1e-9, atol=0)


GEOMETRY = [(0, 2, 300, 3, 0),                                              # as wide as the frame
            (150, 0, 1, 9, 1),                                              # one column
            (10, 4, 200, 1, 0),                                             # one row
            (0, 0, 5, 3, 0), (295, 0, 5, 3, 1), (0, 6, 5, 3, 1), (295, 6, 5, 3, 0)]     # the four corners


def random_boxes(seed, k, cls, xmin=0):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(k):
        bw, bh = int(rng.integers(1, 120)), int(rng.integers(1, H + 1))
        out.append((int(rng.integers(xmin, W - bw + 1)), int(rng.integers(0, H - bh + 1)), bw, bh, cls))
    return out


@pytest.fixture(scope="module")
def main_case():
    """Frame 0: the geometric cases and random boxes, 70 objects (past RTDM_MAX_REGIONS); frame 1: none, between two others;
    frame 2: 95 objects against a capacity of 80, and the only FILTERED pixels of the frame -- its minimum -- inside object 0."""
    disp, masks = frames(11)
    f0 = [o for o in GEOMETRY if o[4] == 0] + random_boxes(1, 32, 0) + [o for o in GEOMETRY if o[4] == 1] + random_boxes(2, 31, 1)
    assert len(f0) == 70
    disp[2][disp[2] == FILTERED] = 48
    disp[2, 2:6, 40:70] = np.where(np.arange(4 * 30).reshape(4, 30) % 3 == 0, FILTERED, disp[2, 2:6, 40:70])
    masks[2, 0, 2:6, 40:70] = 255
    f2 = [(38, 1, 40, 6, 0)] + random_boxes(3, 49, 0, xmin=80) + random_boxes(4, 45, 1, xmin=80)
    assert len(f2) == 95
    lists = [f0, [], f2[:CAP]]
    counts = np.array([[36, 34], [0, 0], [50, 45]], np.int32)
    return disp, masks, lists, counts


def test_main_shape(pkg, oracle, main_case):
    disp, masks, lists, counts = main_case
    want = expect(oracle, disp, masks, lists, counts, CAP)
    got = run(pkg, disp, masks, lists, counts, CAP)
    check(got, want)
    # no assertion above is vacuous: every geometric case, and both classes, hold measured pixels
    for o in GEOMETRY:
        assert want[1][0, lists[0].index(o)] > 0, o
    assert (want[1][0, :70] > 0).sum() >= 60 and (want[1][0, 70:] == NPIX0).all() and (want[0][0, 70:] == MEAN0).all()
    assert (want[1][1] == NPIX0).all() and (got[0][1] == MEAN0).all()       # the frame without objects
    assert (want[1][2] != NPIX0).all() and (want[1][2] > 0).sum() >= 70     # 95 against 80: every entry written, nothing past them
    # the frame whose minimum lies only inside object 0: the pixels at that minimum are not measured there
    x, y, bw, bh, _ = lists[2][0]
    inside = (masks[2, 0, y:y + bh, x:x + bw] != 0)
    assert (disp[2] == FILTERED).sum() == 40 and want[1][2, 0] == inside.sum() - 40
    assert all(o[0] >= 80 for o in lists[2][1:]) and (disp[2, :, 80:] != FILTERED).all()


def test_more_objects_than_capacity(pkg, oracle, main_case):
    """95 and 70 counted objects against capacities of 80 and 60: the first `capacity` are measured and nothing behind them is
    written -- the frame of 95 lies first, so what overran its row would land in the empty frame's sentinels behind it."""
    disp, masks, lists, counts = main_case
    order = [2, 1, 0]
    for cap in (CAP, 60):
        cut = [lists[f][:cap] for f in order]
        got = run(pkg, disp[order], masks[order], cut, counts[order], cap)
        check(got, expect(oracle, disp[order], masks[order], cut, counts[order], cap))
        assert (got[1][0] != NPIX0).all() and (got[1][1] == NPIX0).all() and (got[0][1] == MEAN0).all()
        assert (got[1][2] != NPIX0).sum() == min(70, cap) and (got[0][2] != MEAN0).sum() == min(70, cap)


def test_a_class_whose_own_plane_is_empty(pkg, oracle):
    disp, masks = frames(12, n=1)
    masks[0, 0], masks[0, 1] = 255, 0
    lists, counts = [[(20, 1, 60, 7, 0), (20, 1, 60, 7, 1)]], np.array([[1, 1]], np.int32)
    mean, npix = run(pkg, disp, masks, lists, counts, CAP)
    check((mean, npix), expect(oracle, disp, masks, lists, counts, CAP))
    assert npix[0, 0] > 0 and mean[0, 0] > 0 and npix[0, 1] == 0 and mean[0, 1] == 0.0


def test_padded_pitches_and_strides(pkg, oracle, main_case):
    disp, masks, lists, counts = main_case
    check(run(pkg, disp, masks, lists, counts, CAP, padded=True), expect(oracle, disp, masks, lists, counts, CAP))


def test_untrusted_lists(pkg, oracle):
    """D4: boxes that leave the frame are measured as their clipped part; empty boxes, foreign classes and a negative count
    finish clean."""
    disp, masks = frames(13, n=2)
    big = 2 ** 31 - 1
    f0 = [(-5, -2, 20, 6, 0), (290, 5, 50, 50, 1), (10, 2, -4, 3, 0), (400, 2, 5, 5, 0), (5, 20, 3, 3, 1), (3, 3, 10, 4, 9),
          (3, 3, 10, 4, -1), (big - 40, 1, big - 40, 3, 0), (-big - 1, 0, big, 5, 1), (-big - 1, -big - 1, big, big, 0),
          (10, 1, big, big, 1), (0, 0, 0, 0, 0)]
    f1 = [(-1, -1, W + 2, H + 2, 1)]
    lists = [f0, f1]
    counts = np.array([[-5, len(f0)], [1, -(2 ** 31)]], np.int32)             # negative counts count as 0
    want = expect(oracle, disp, masks, lists, counts, CAP)
    got = run(pkg, disp, masks, lists, counts, CAP)
    check(got, want)
    assert clip(f0[0]) == (0, 0, 15, 4) and clip(f0[1]) == (290, 5, 10, 4) and clip(f0[10]) == (10, 1, 290, 8) and clip(f1[0]) == (0, 0, W, H)
    assert all(want[1][0, i] > 0 for i in (0, 1, 10)) and want[1][1, 0] > 0
    assert all(want[1][0, i] == 0 and want[0][0, i] == 0.0 for i in (2, 3, 4, 5, 6, 7, 8, 9, 11))
    assert (got[1][0, len(f0):] == NPIX0).all() and (got[1][1, 1:] == NPIX0).all()


def test_order_of_summation_is_fixed(pkg, main_case):
    """D3: two runs, the frame alone, the frame at another position of another batch, another capacity: the same bits."""
    disp, masks, lists, counts = main_case
    a, b = run(pkg, disp, masks, lists, counts, CAP, two=True)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    alone = run(pkg, disp[0:1], masks[0:1], lists[0:1], counts[0:1], CAP)
    moved = run(pkg, disp[[2, 1, 0]], masks[[2, 1, 0]], [lists[2], lists[1], lists[0]], counts[[2, 1, 0]], CAP)
    wide = run(pkg, disp[0:1], masks[0:1], lists[0:1], counts[0:1], 200)
    k = 70
    for mean, npix in ((alone[0][0], alone[1][0]), (moved[0][2], moved[1][2]), (wide[0][0], wide[1][0])):
        assert mean[:k].tobytes() == a[0][0, :k].tobytes() and npix[:k].tobytes() == a[1][0, :k].tobytes()
        assert (npix[k:] == NPIX0).all()
    assert moved[0][0].tobytes() == a[0][2].tobytes()


def test_against_the_single_frame_call(pkg, main_case):
    import torch
    disp, masks, lists, counts = main_case
    mean, npix = run(pkg, disp, masks, lists, counts, CAP)
    for f, c in ((0, 0), (0, 1), (2, 1)):
        idx = [i for i, o in enumerate(lists[f]) if o[4] == c][:64]
        assert 30 <= len(idx) <= 64
        m1, n1 = pkg.depth_stats_device(torch.from_numpy(disp[f]).cuda(), Q, torch.from_numpy(np.ascontiguousarray(masks[f, c])).cuda(),
                                        [lists[f][i][:4] for i in idx])
        assert np.array_equal(n1, npix[f, idx]) and n1.sum() > 0
        np.testing.assert_allclose(mean[f, idx], m1, rtol=1e-9, atol=0)


@pytest.mark.parametrize("labels", [False, True])
def test_the_walk_of_a_box_is_rule_d3(pkg, labels):
    """D3 bit for bit: mean and npix of every box of tests/d3_walk_model.py's scene equal the model's lane-by-lane, band-by-band
    float64 sums.  On that scene the order shows: tests/test_d3_walk_model_cpu.py holds that a row-major sum, another fold of the
    lanes or the bands in descending order each change the bits of this mean in several boxes."""
    disp, mask, planes, boxes = d3.scene()
    plane = planes if labels else mask
    k = len(boxes)
    want_mean, want_npix = d3.depth_model(disp, plane[0], boxes, labels)
    assert k == d3.CAP - 1 and (want_npix > 0).sum() >= k - 6 and (want_mean != 0).sum() == (want_npix > 0).sum()
    mean, npix = run(pkg, disp[None], plane[None], [boxes], np.array([[k]], np.int32), d3.CAP, labels=labels, q=d3.Q)
    assert npix[0, :k].tobytes() == want_npix.tobytes(), np.argwhere(npix[0, :k] != want_npix)[:8]
    assert mean[0, :k].tobytes() == want_mean.tobytes(), np.argwhere(mean[0, :k] != want_mean)[:8]
    assert (npix[0, k:] == NPIX0).all() and (mean[0, k:] == MEAN0).all()
