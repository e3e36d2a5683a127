"""The case list of tests/test_gpu_morph_general.py and the inputs that go with every case, shared with
tests/test_morph_general_cpu.py, which walks the same list without a device.

Every case gets inputs whose REFERENCE result (tests/morph_ref.py) is neither constant nor equal to the input, so that no
case passes on a frame that a broken kernel would also get right.  pick() takes the first of a fixed list of candidate
frames that meets this: for gray frames a low-frequency ramp plus noise; for masks a clean solid block and a clean empty
block, each as wide as the element's reach over all iterations (or half the frame), with blobs and salt and pepper between
them, the solid block at the left, right, top or bottom; last, for frames of a few pixels, frames with one odd pixel.
The condition is dropped only where the geometry makes it impossible (forced()): a single erosion or dilation whose
windows, clipped to the frame, are the same set for every pixel (a constant whatever the input: ELLIPSE 63x63 on 5x3) or
hold nothing but the pixel itself (the input: a single-member element such as ELLIPSE 9x1, a column element on a one-row
frame, any element on the 1x1 frame).  Anything else for which no candidate works is an error of this file and raises."""
import numpy as np

import morph_ref as mr

FRAMES = [(1, 1), (5, 3), (63, 1), (64, 32), (65, 33), (97, 65), (233, 156)]
SIZES = [(1, 1), (2, 2), (3, 3), (10, 10), (7, 4), (1, 9), (9, 1), (31, 31), (63, 63), (63, 2)]
NAMED = [(shape, w, h) for shape in (mr.RECT, mr.CROSS, mr.ELLIPSE) for (w, h) in SIZES]
RANDOM_SIZES = [(9, 6), (5, 13), (17, 3), (33, 20), (63, 63), (4, 4)]
ELEMENTS_FOR_OPS = [("rect3", mr.element(mr.RECT, 3, 3), None), ("ellipse10", mr.element(mr.ELLIPSE, 10, 10), None),
                    ("cross7x4", mr.element(mr.CROSS, 7, 4), None), ("random9x6", mr.random_element(9, 6, 77), (8, 0)),
                    ("ellipse31", mr.element(mr.ELLIPSE, 31, 31), None)]


def _offsets(el, anchor):
    el = np.asarray(el) != 0
    kh, kw = el.shape
    ax, ay = (kw // 2, kh // 2) if anchor is None else anchor
    return [(int(i) - ay, int(j) - ax) for i, j in zip(*np.nonzero(el))]


def forced(W, H, el, anchor):
    """Is the result of ONE erosion / dilation constant, or the input, for every W x H input?  From the geometry alone."""
    inside = [(dy, dx) for dy, dx in _offsets(el, anchor) if abs(dy) < H and abs(dx) < W]     # offsets that can land in the frame
    if set(inside) <= {(0, 0)}:
        return True                                                   # nothing but the pixel itself (or nothing at all)
    seen = np.zeros((H, W), np.int64)                                 # seen[q] = pixels whose clipped window holds q
    for dy, dx in inside:
        seen[max(0, dy):min(H, H + dy), max(0, dx):min(W, W + dx)] += 1
    return bool(np.isin(seen, (0, W * H)).all())                      # every window is the same set


def nontrivial(want, frame):
    return want.min() != want.max() and not np.array_equal(want, frame)


def _mask_layout(W, H, seed, reach_x, reach_y, layout):
    rng = np.random.default_rng(seed)
    n, reach = (W, reach_x) if layout < 2 else (H, reach_y)
    r = min(reach, n // 2)
    yy, xx = np.mgrid[0:H, 0:W]
    m = np.zeros((H, W), bool)
    for _ in range(max(2, W * H // 900)):
        cx, cy, rad = rng.integers(0, W), rng.integers(0, H), rng.integers(2, 3 + max(W, H) // 4)
        m |= (xx - cx) ** 2 + (yy - cy) ** 2 <= rad * rad
    m ^= rng.random((H, W)) < 0.04
    along = xx if layout < 2 else yy
    m[along < r] = True                                               # clean solid block
    m[along >= n - r] = False                                         # clean empty block
    if layout & 1:
        m = m[::-1, ::-1]
    return (np.ascontiguousarray(m) * 255).astype(np.uint8)


def _odd_pixel(W, H, y, x, base, odd):
    f = np.full((H, W), base, np.uint8)
    f[y, x] = odd
    return f


def candidates(kind, W, H, el, it, seed):
    kh, kw = np.asarray(el).shape
    if kind == "gray":
        yield mr.gray_frame(W, H, seed)
        yield mr.gray_frame(W, H, seed + 100)[::-1, ::-1].copy()
        base, odds = 120, (20, 230)
    else:
        for layout in range(4):
            yield _mask_layout(W, H, seed, it * kw, it * kh, layout)
        base, odds = None, (0, 255)
    for y, x in ((0, 0), (H - 1, W - 1), (0, W - 1), (H - 1, 0), (H // 2, W // 2)):
        for odd in odds:
            yield _odd_pixel(W, H, y, x, (255 - odd) if base is None else base, odd)


def pick(kind, W, H, el, anchor, op, it, seed):
    """-> (frame, reference result, whether the result is neither constant nor the frame)"""
    first = None
    for f in candidates(kind, W, H, el, it, seed):
        want = mr.morphology(f, op, el, anchor, it)
        if nontrivial(want, f):
            return f, want, True
        if first is None:
            first = (f, want, False)
    assert op in (mr.ERODE, mr.DILATE) and forced(W, H, el, anchor), \
        ("no candidate input gives a result that is neither constant nor the input", kind, W, H, np.asarray(el).shape, anchor, op, it)
    return first


def _case(W, H, el, anchor, op, it, kinds):
    frames = [pick(kind, W, H, el, anchor, op, it, seed) for kind, seed in kinds]
    return dict(W=W, H=H, el=el, anchor=anchor, op=op, it=it, frames=[f for f, _, _ in frames], want=[w for _, w, _ in frames],
                asserted=[a for _, _, a in frames])


def named_cases(shape, w, h):
    el = mr.element(shape, w, h)
    for W, H in FRAMES:
        for op in (mr.ERODE, mr.DILATE):
            yield _case(W, H, el, None, op, 1, [("gray", 3), ("gray", 4), ("mask", 5)])


def random_cases(seed):
    w, h = RANDOM_SIZES[seed]
    el = mr.random_element(w, h, seed)
    for W, H in [(65, 33), (97, 65), (5, 3)]:
        for anchor in [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (w // 3, h // 2)]:
            for op in (mr.ERODE, mr.DILATE):
                yield _case(W, H, el, anchor, op, 1, [("gray", 10 + seed), ("mask", 20 + seed)])


def op_cases(op):
    for W, H in [(65, 33), (97, 65)]:
        for name, el, anchor in ELEMENTS_FOR_OPS:
            for it in (1, 2, 3):
                if name == "ellipse31" and it > 1:
                    continue
                yield _case(W, H, el, anchor, op, it, [("gray", 30), ("mask", 31), ("gray", 32)])


def aligned_cases(op):
    for W, H in [(256, 128), (260, 100)]:
        for name, el, anchor in ELEMENTS_FOR_OPS:
            yield _case(W, H, el, anchor, op, 1, [("gray", 70), ("mask", 71), ("gray", 72)])
