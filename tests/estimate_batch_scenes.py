"""The frames of tests/test_gpu_estimate_batch.py and what the CPU oracle says of them: rectify_util.red_scene with the objects
of the right half turned blue, exactly as two_colour_scene in tests/test_gpu_objects_batch.py does it, for any seed."""
import numpy as np

import objects_batch_ref as ref
import rectify_util as ru

BLUE_LOW, BLUE_HIGH = (110, 150, 0), (130, 255, 255)
D, BLOCK, MIN_AREA = 32, 7, 40


def two_colour_scene(synth, c, seed):
    left, right = ru.red_scene(synth, seed, c["W"], c["H"], D)
    for img in (left, right):
        half = img[:, c["W"] // 2:]
        red = (half[..., 0] > half[..., 1])
        half[red] = half[red][:, ::-1]
    return left, right


def gray_pair(left):
    """A frame pair without an object of either class."""
    g = np.ascontiguousarray(np.stack([left[..., 1]] * 3, -1))
    return g, g.copy()


def ranges(oracle):
    return [(oracle.HSV_LOW, oracle.HSV_HIGH), (BLUE_LOW, BLUE_HIGH)]


def detect(oracle, c, maps, left):
    """objects_batch_ref.detect on the rectified colour crop of `left`, with the reference's filter."""
    col = oracle.rectify_rgb(left, maps[0], maps[1], c["roi"])
    return ref.detect(oracle, col, ranges(oracle), None, MIN_AREA, True, oracle.morph_open_close)


def oracle_chain(oracle, c, maps, left, right, capacity):
    """The whole chain on the CPU -> (objects, counts, mean_cm, npix, disp) with no limit of 64 on the measured objects."""
    want = detect(oracle, c, maps, left)
    gl = oracle.rectify_gray(left, maps[0], maps[1], c["roi"]); gr = oracle.rectify_gray(right, maps[2], maps[3], c["roi"])
    disp = oracle.bm_compute(gl, gr, numDisparities=D, blockSize=BLOCK, roi1=want["roi"], nthreads=8)
    mean, cnt = ref.depth(oracle, disp, c["Q"], want["masks"], want["objects"], capacity, max_regions=capacity)
    return want["objects"][:capacity], want["counts"], mean, cnt, disp
