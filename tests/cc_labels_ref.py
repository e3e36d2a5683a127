"""Reference for the detector's label planes, pixel moments and own-pixel depth (rules L1, L2 and L5 of DESIGN.md section
4.17): bruteforce.external_boxes -- scipy.ndimage labelling -- extended to say WHICH pixels belong to every kept object.
Shared by tests/test_objects_labels_cpu.py and tests/test_gpu_objects_labels.py.  Moments are integer sums (numpy int64; the
largest, below W * H * max(W, H)^2, is far below 2^63 at every size the detector serves)."""
import numpy as np

MOMENTS = ("m00", "m10", "m01", "m20", "m11", "m02")


def kept_components(mask, min_area=100, zero_border=True):
    """bruteforce.external_boxes with its components: -> (kept, fg): kept = [(first pixel, (x, y, w, h), scipy label)] in O4
    order (first pixel descending), fg = the 8-connected labelling of the filtered plane's foreground."""
    from scipy import ndimage as ndi
    m = np.asarray(mask) != 0
    if zero_border:
        m = m.copy(); m[0, :] = m[-1, :] = False; m[:, 0] = m[:, -1] = False
    H, W = m.shape
    pad = np.zeros((H + 2, W + 2), bool); pad[1:-1, 1:-1] = m
    bg, _ = ndi.label(~pad)                                   # 4-connected by default
    outer = bg == bg[0, 0]
    near_outer = ndi.binary_dilation(outer, structure=ndi.generate_binary_structure(2, 1))[1:-1, 1:-1]
    fg, n = ndi.label(m, structure=np.ones((3, 3), bool))      # 8-connected
    flat = fg.ravel()
    first = np.full(n + 1, flat.size, np.int64)
    np.minimum.at(first, flat, np.arange(flat.size))
    external = np.zeros(n + 1, bool)
    external[np.unique(fg[near_outer & m])] = True
    kept = []
    for i, sl in enumerate(ndi.find_objects(fg), 1):
        if not external[i]:
            continue
        ys, xs = sl
        box = (xs.start, ys.start, xs.stop - xs.start, ys.stop - ys.start)
        if box[2] * box[3] >= min_area:
            kept.append((int(first[i]), box, i))
    return sorted(kept, reverse=True), fg


def moments(labels, count):
    """labels: int32 H x W with values 0 .. count -> int64 [count, 6]: Σ1, Σx, Σy, Σx², Σxy, Σy² over the pixels of 1 .. count."""
    H, W = labels.shape
    ys, xs = np.nonzero(labels)
    ids = labels[ys, xs].astype(np.int64)
    xs, ys = xs.astype(np.int64), ys.astype(np.int64)
    out = np.zeros((count + 1, 6), np.int64)
    for k, w in enumerate((np.ones_like(xs), xs, ys, xs * xs, xs * ys, ys * ys)):
        np.add.at(out[:, k], ids, w)                           # integer adds: exact
    return out[1:]


def frame(masks, min_area=100, zero_border=True, capacity=1 << 30):
    """The filtered class planes of one frame -> dict(objects [(x, y, w, h, cls)] unclipped, first_pixels, counts [K], stored,
    labels int32 K x H x W (L1 for `capacity`), stats int64 [stored, 6] (L2))."""
    objects, firsts, counts, comps = [], [], [], []
    for c, m in enumerate(masks):
        kept, fg = kept_components(m, min_area, zero_border)
        objects += [box + (c,) for _, box, _ in kept]
        firsts += [f for f, _, _ in kept]
        counts.append(len(kept))
        comps.append((kept, fg))
    stored = min(len(objects), capacity)
    labels = np.zeros((len(masks),) + np.asarray(masks[0]).shape, np.int32)
    stats = np.zeros((stored, 6), np.int64)
    base = 0
    for c, (kept, fg) in enumerate(comps):
        lut = np.zeros(int(fg.max()) + 1, np.int32)
        for j, (_, _, comp) in enumerate(kept):
            if base + j < stored:
                lut[comp] = base + j + 1
        labels[c] = lut[fg]
        base += len(kept)
    for c in range(len(masks)):
        stats += moments(labels[c], stored)
    return dict(objects=objects, first_pixels=firsts, counts=counts, stored=stored, labels=labels, stats=stats)


def clipped(o, W, H):
    x, y, w, h = o[:4]
    x0, y0, x1, y1 = max(x, 0), max(y, 0), min(x + w, W), min(y + h, H)
    return (x0, y0, x1 - x0, y1 - y0) if w > 0 and h > 0 and x1 > x0 and y1 > y0 else None


def contaminated(masks, labels, objects, stored):
    """Per stored object: does its box hold foreground of its class plane that is not its own (what rule D1 would add)?"""
    out = []
    for i, (x, y, w, h, c) in enumerate(objects[:stored]):
        box = (slice(y, y + h), slice(x, x + w))
        out.append(bool(((np.asarray(masks[c])[box] != 0) & (labels[c][box] != i + 1)).any()))
    return out


def depth_own(oracle, disp16, Q, labels, objects, stored, calibration_unit=25.0):
    """L5: oracle.depth_stats once per stored object, under the mask (labels == i + 1) * 255 of its class plane and over its
    own box -> (mean_cm [stored], npix [stored])."""
    mean = np.zeros(stored, np.float64)
    npix = np.zeros(stored, np.int32)
    for i, o in enumerate(objects[:stored]):
        own = ((labels[o[4]] == i + 1) * 255).astype(np.uint8)
        m, k = oracle.depth_stats(disp16, Q, own, [o[:4]], calibration_unit)
        mean[i], npix[i] = m[0], k[0]
    return mean, npix
