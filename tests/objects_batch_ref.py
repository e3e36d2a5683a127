"""Reference for the batched, multi-class object detection (rules O1-O4 of DESIGN.md section 4.15), built from the
oracle's single-mask pieces only: oracle.hsv_inrange, numpy OR, a filter given by the caller (identity, tests/morph_ref.py or
oracle.morph_open_close), oracle.external_boxes, oracle.union_box and oracle.depth_stats.  Shared by
tests/test_objects_batch_cpu.py and tests/test_gpu_objects_batch.py."""
import numpy as np

ALL_BOXES = 1 << 16                       # above every box count the tests produce

RED, BLUE, GREEN, GRAY = (200, 20, 20), (20, 20, 200), (20, 200, 20), (128, 128, 128)
# single-interval ranges that hold exactly one of the three colours above (h = 0, 120, 60; s = 229; v = 200)
R_RED, R_BLUE, R_GREEN = ((0, 150, 0), (9, 255, 255)), ((110, 150, 0), (130, 255, 255)), ((50, 150, 0), (70, 255, 255))
# two classes that may share pixels: class 0 = red OR green, class 1 = blue OR green
TWO_RANGES, TWO_CLASSES = [R_RED, R_GREEN, R_BLUE, R_GREEN], [0, 0, 1, 1]


def paint2(mask_a, mask_b):
    """RGB frame whose raw masks under TWO_RANGES / TWO_CLASSES are exactly mask_a (class 0) and mask_b (class 1)."""
    a, b = np.asarray(mask_a) != 0, np.asarray(mask_b) != 0
    rgb = np.empty(a.shape + (3,), np.uint8)
    rgb[...] = GRAY
    rgb[a & ~b] = RED
    rgb[b & ~a] = BLUE
    rgb[a & b] = GREEN
    return rgb


def class_ids(ranges, classes):
    classes = list(range(len(ranges))) if classes is None else list(classes)
    assert len(classes) == len(ranges) and sorted(set(classes)) == list(range(max(classes) + 1)), "every class owns a range"
    return classes, max(classes) + 1


def raw_masks(oracle, rgb, ranges, classes=None):
    """O1: per class the OR of its ranges' inRange results."""
    classes, K = class_ids(ranges, classes)
    H, W, _ = rgb.shape
    out = [np.zeros((H, W), np.uint8) for _ in range(K)]
    for (lo, hi), c in zip(ranges, classes):
        out[c] |= oracle.hsv_inrange(rgb, lo, hi)
    return out


def identity(mask):
    return mask


def detect(oracle, rgb, ranges, classes=None, min_area=100, zero_border=True, filt=identity):
    """O1-O4 for one frame -> dict(masks: K filtered planes, objects: [(x, y, w, h, cls)] unclipped, counts: K ints,
    roi: (x, y, w, h))."""
    masks = [np.ascontiguousarray(filt(m)) for m in raw_masks(oracle, rgb, ranges, classes)]
    objects, counts = [], []
    for c, m in enumerate(masks):
        boxes = oracle.external_boxes(m, min_area, zero_border, max_boxes=ALL_BOXES)
        assert len(boxes) < ALL_BOXES
        objects += [b + (c,) for b in boxes]
        counts.append(len(boxes))
    return dict(masks=masks, objects=objects, counts=counts, roi=oracle.union_box([o[:4] for o in objects]))


def depth(oracle, disp16, Q, masks, objects, max_objects, calibration_unit=25.0, max_regions=64):
    """The chain's last step: the first min(len, max_objects, max_regions) objects, each under its own class's mask."""
    objs = objects[:min(len(objects), max_objects, max_regions)]
    mean = np.zeros(len(objs), np.float64)
    cnt = np.zeros(len(objs), np.int32)
    for c in sorted(set(o[4] for o in objs)):
        idx = [i for i, o in enumerate(objs) if o[4] == c]
        m, n = oracle.depth_stats(disp16, Q, masks[c], [objs[i][:4] for i in idx], calibration_unit)
        mean[idx] = m
        cnt[idx] = n
    return mean, cnt
