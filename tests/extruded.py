"""Extruded stereo pairs -- every row of a band is the same row -- and the analysis that says what a disparity map of
such a pair asks of the speckle filter.  A helper: no test in here, nothing imported from the kernels.

A band is a 1-D random signal s and a disparity profile d(x) = d0 + slope * x: the right row is s(x), the left row is
s(x - d(x)) by linear interpolation, rounded to uint8, and the row is repeated.  Block matching returns the same disparity
row on every interior row of the band, so every pixel is in vertical contact with the pixel above it, while `slope` and
speckleRange set how long the horizontal runs are.  Bands with different signals agree on the true disparity but differ in
quantisation noise and in the pixels the left-right check kills: long runs of one band sit on thin columns of the next.

The analysis functions take an UNFILTERED int16 map d (speckleWindowSize = 0), the filtered value FIL and maxDiff in the
map's own 1/16 units (speckleRange for StereoBM, 16 * speckleRange for StereoSGBM).
"""
import numpy as np


def band_rows(rng, W, D, d0, slope):
    """-> (left_row, right_row), uint8 [W].  rng: numpy Generator.  Where d(x) = d0 + slope * x leaves the search range
    [0, D) the matcher finds no true match and returns what it likes -- still the same on every row."""
    x = np.arange(W, dtype=np.float64)
    dx = d0 + slope * x
    assert dx.min() >= 0, (d0, slope)
    pad = int(np.ceil(dx.max())) + 2
    n = W + pad
    s = rng.integers(0, 256, n + 2).astype(np.float64)
    s = (s[:-2] + 2.0 * s[1:-1] + s[2:]) / 4.0           # one binomial pass: linear interpolation keeps some contrast
    s = np.clip((s - 128.0) * 1.6 + 128.0, 0.0, 255.0)
    pos = x - dx + pad                                    # >= 0: s carries `pad` samples left of column 0
    i0 = np.floor(pos).astype(np.int64)
    fr = pos - i0
    left = s[i0] * (1.0 - fr) + s[i0 + 1] * fr
    right = s[pad:pad + W]
    return np.rint(left).astype(np.uint8), np.rint(right).astype(np.uint8)


def banded(seed, W, D, bands):
    """bands = [(rows, d0, slope), ...] -> contiguous uint8 (L, R) of sum(rows) x W."""
    rng = np.random.default_rng(seed)
    Ls, Rs = [], []
    for rows, d0, slope in bands:
        l, r = band_rows(rng, W, D, d0, slope)
        Ls.append(np.repeat(l[None], rows, axis=0)); Rs.append(np.repeat(r[None], rows, axis=0))
    return np.ascontiguousarray(np.concatenate(Ls)), np.ascontiguousarray(np.concatenate(Rs))


def _edges(d, FIL, maxDiff):
    d = np.asarray(d).astype(np.int64)
    v = d != FIL
    eh = v[:, 1:] & v[:, :-1] & (np.abs(d[:, 1:] - d[:, :-1]) <= maxDiff)       # eh[y, x]: (y, x) - (y, x + 1)
    ev = v[1:, :] & v[:-1, :] & (np.abs(d[1:, :] - d[:-1, :]) <= maxDiff)       # ev[y, x]: (y, x) - (y + 1, x)
    return v, eh, ev


def new_run_contacts(d, FIL, maxDiff):
    """Boolean map: (y, x) touches (y - 1, x) and that contact is not the continuation of the contact to its left -- the
    left one joins the same two runs iff it is a contact too and neither (y, x) nor (y - 1, x) starts a horizontal run.
    One union per True.  Row 0 is False."""
    v, eh, ev = _edges(d, FIL, maxDiff)
    H, W = v.shape
    start = v.copy()                                       # start[y, x]: (y, x) starts a run
    start[:, 1:] &= ~eh
    c = np.zeros((H, W), bool)
    c[1:] = ev
    left = np.zeros((H, W), bool)
    left[:, 1:] = c[:, :-1]
    above_start = np.zeros((H, W), bool)
    above_start[1:] = start[:-1]
    return c & ~(left & ~start & ~above_start)


def max_contacts_per_workgroup(cand, rows, rs=1):
    """Largest number of new-run contacts one workgroup of 256 threads meets: a thread takes one chunk of 8 columns, the
    chunks are numbered row-major over `rows` (the lower rows of the row pairs a kernel numbers that way), a workgroup
    takes 256 consecutive numbers from a multiple of 256.  rs > 1: a thread walks a strip of rs consecutive entries of
    `rows` in its 8 columns, and the strips are what is numbered."""
    cand = np.asarray(cand)
    rows = list(rows)
    if not rows:
        return 0
    W = cand.shape[1]
    nxb = (W + 7) // 8
    ns = (len(rows) + rs - 1) // rs
    c = np.zeros((ns * rs, nxb * 8), np.int64)
    c[:len(rows), :W] = cand[rows]
    per = c.reshape(ns, rs, nxb, 8).sum(axis=(1, 3)).ravel()
    per = np.concatenate([per, np.zeros(-len(per) % 256, np.int64)])
    return int(per.reshape(-1, 256).sum(axis=1).max())


def components(d, FIL, maxDiff):
    """4-neighbour components of the valid pixels under |a - b| <= maxDiff -> (label map, -1 where invalid; sizes by label)."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    v, eh, ev = _edges(d, FIL, maxDiff)
    H, W = v.shape
    idx = np.arange(H * W).reshape(H, W)
    a = np.concatenate([idx[:, :-1][eh], idx[:-1, :][ev]])
    b = np.concatenate([idx[:, 1:][eh], idx[1:, :][ev]])
    g = coo_matrix((np.ones(len(a), np.int8), (a, b)), shape=(H * W, H * W))
    _, lab = connected_components(g, directed=False)
    lab = lab.reshape(H, W)
    sizes = np.bincount(lab[v], minlength=H * W)
    return np.where(v, lab, -1), sizes


def filter_by_components(d, FIL, maxDiff, win):
    """cv::filterSpeckles from components(): a component of at most `win` pixels becomes FIL."""
    lab, sizes = components(d, FIL, maxDiff)
    out = np.array(d, np.int16, copy=True)
    out[(lab >= 0) & (sizes[np.maximum(lab, 0)] <= win)] = FIL
    return out


def run_lengths(d, FIL, maxDiff):
    """Per pixel: the length of its horizontal run (0 where invalid)."""
    v, eh, _ = _edges(d, FIL, maxDiff)
    H, W = v.shape
    start = v.copy()
    start[:, 1:] &= ~eh
    rid = np.cumsum(start.ravel()).reshape(H, W)           # run ids ascend along a row and never repeat across rows
    ln = np.bincount(rid[v], minlength=int(rid.max()) + 1)
    return np.where(v, ln[rid], 0)


def rescue_depth(d, FIL, maxDiff, win):
    """-> (pixels in runs <= win whose component holds a run > win, the largest row distance from such a pixel to the
    nearest row where its component has a long run).  These pixels survive the filter only through what the long run's
    contacts hand on, row by row."""
    lab, sizes = components(d, FIL, maxDiff)
    ln = run_lengths(d, FIL, maxDiff)
    H, W = lab.shape
    long_px = ln > win
    has_long = np.zeros(len(sizes), bool)
    has_long[lab[long_px]] = True
    resc = (lab >= 0) & ~long_px & has_long[np.maximum(lab, 0)]
    if not resc.any():
        return 0, 0
    depth = 0
    ys = np.arange(H)
    for c in np.unique(lab[resc]):
        long_rows = np.unique(np.nonzero(long_px & (lab == c))[0])
        need_rows = np.unique(np.nonzero(resc & (lab == c))[0])
        dist = np.abs(need_rows[:, None] - long_rows[None, :]).min(axis=1)
        depth = max(depth, int(dist.max()))
    del ys
    return int(resc.sum()), depth


def band_height(d, FIL, y0, y1):
    """Height of a band's columns, read off the map: the tallest column of valid pixels in rows [y0, y1)."""
    return int((np.asarray(d)[y0:y1] != FIL).sum(axis=0).max())


# ---- the inputs the speckle tests use, with the conditions that keep them from passing while exercising nothing ------------
# Everything below runs on the CPU oracle alone; test_extruded_cpu.py and the GPU cases call the same functions, so an
# input that drifts fails on a machine without a GPU first.
BM = dict(numDisparities=32, blockSize=9, uniquenessRatio=0, textureThreshold=0)
QCAP = 1024                       # the merge kernels' LDS union queue
OVERFLOW_MIN = 1280               # 1.25 x the queue
RESCUED_MIN, DEPTH_MIN = 2000, 12
ONE_BAND = [(40, 3, 0.06)]
THREE_BANDS_03 = [(24, 3, 0.03), (40, 3, 0.03), (24, 3, 0.03)]
THREE_BANDS_01 = [(24, 3, 0.01), (40, 3, 0.01), (24, 3, 0.01)]
MARK_CASES = [(THREE_BANDS_03, 0, 3), (THREE_BANDS_03, 0, 2), (THREE_BANDS_01, 1, 8), (THREE_BANDS_01, 1, 20),
              (THREE_BANDS_01, 2, 20)]               # (bands, speckleRange, window), disp12MaxDiff = 1
# (H, y offset of ROI1): blockSize 9 computes vy1 - vy0 = H - 8 - offset rows = 1 .. 9 and 33.  cv::StereoBM refuses
# blockSize >= H, so a single row comes from H = 10 with one row cut by the ROI.
BLOCK_HEIGHTS = [(10, 1)] + [(H, 0) for H in range(10, 18)] + [(41, 0)]
ROI_HEIGHT, ROI_OFFSETS = 24, (0, 1, 2, 3)           # vy0 = 4 + offset, vy1 - vy0 = 16 - offset
BATCH_SEEDS = (11, 12, 13, 14)


def fil(kw):
    return (kw.get("minDisparity", 0) - 1) * 16


def unfiltered(orc, L, R, **kw):
    return orc.bm_compute(L, R, nthreads=8, **dict(kw, speckleWindowSize=0))


def checked_rows(orc, L, kw):
    """(vy0, vy1): the rows the matcher computes"""
    H, W = L.shape
    vr = orc.valid_rect(W, H, **{k: v for k, v in kw.items() if k not in ("speckleWindowSize",)})
    return vr[1], vr[1] + vr[3]


def pair_rows(vy0, vy1, which="all"):
    """Lower rows of the row pairs a merge kernel numbers row-major: every pair; the pairs inside blocks of four rows from
    vy0 (the head records' contacts); the pairs across those blocks."""
    ys = range(vy0 + 1, vy1)
    if which == "all":
        return list(ys)
    return [y for y in ys if ((y - vy0) % 4 != 0) == (which == "inside")]


def require_overflow(d, FIL, maxDiff, vy0, vy1):
    cand = new_run_contacts(d, FIL, maxDiff)
    got = {w: max_contacts_per_workgroup(cand, pair_rows(vy0, vy1, w)) for w in ("all", "inside")}
    assert min(got.values()) >= OVERFLOW_MIN, ("a workgroup must meet 1.25 x the union queue", got)
    return got


def require_hv_boundary(orc, d, FIL, maxDiff, hv):
    a, b = orc.filter_speckles(d, FIL, hv - 1, maxDiff), orc.filter_speckles(d, FIL, hv, maxDiff)
    n = int((a != b).sum())
    assert n >= 1000, ("windows hv - 1 and hv must differ in 1000 pixels", hv, n)
    return n


def require_rescue(d, FIL, maxDiff, win):
    n, depth = rescue_depth(d, FIL, maxDiff, win)
    assert n >= RESCUED_MIN and depth >= DEPTH_MIN, ("rescued pixels / depth", win, n, depth)
    return n, depth


def require_exact_sizes(d, FIL, maxDiff, win):
    lab, sizes = components(d, FIL, maxDiff)
    sz = np.where(lab >= 0, sizes[np.maximum(lab, 0)], 0)
    at, above = int((sz == win).sum()), int((sz == win + 1).sum())
    assert at >= 100 and above >= 100, ("pixels in components of exactly window / window + 1", win, at, above)
    return at, above


def require_every_pair_in_contact(d, FIL, maxDiff, vy0, vy1, hv):
    """the block-arithmetic inputs: every row pair carries contacts and columns survive window hv only as part of wider
    components, so a pair that no kernel merges changes which pixels survive"""
    cand = new_run_contacts(d, FIL, maxDiff)
    assert all(cand[y].sum() >= 50 for y in range(vy0 + 1, vy1)), "a row pair without contacts"
    lab, sizes = components(d, FIL, maxDiff)
    sz = np.where(lab >= 0, sizes[np.maximum(lab, 0)], 0)
    gone, kept = int(((sz > 0) & (sz <= hv)).sum()), int((sz > hv).sum())
    assert gone >= 50 * hv and kept >= 8 * hv, (hv, gone, kept)
    return gone, kept


def _job(orc, name, L, R, kw, wins, bands=None):
    d = unfiltered(orc, L, R, **kw)
    FIL = fil(kw)
    vy0, vy1 = checked_rows(orc, L, kw)
    hv = band_height(d, FIL, 0, L.shape[0])
    return dict(name=name, L=L, R=R, kw=kw, d=d, FIL=FIL, maxDiff=kw["speckleRange"], vy0=vy0, vy1=vy1, hv=hv,
                windows=[w(hv) if callable(w) else w for w in wins], bands=bands, measured={})


HV_WINDOWS = (lambda hv: hv - 1, lambda hv: hv, lambda hv: 2 * hv - 1, lambda hv: 2 * hv)


def overflow_jobs(orc):
    """Case 1: one band whose every workgroup of the compact-head merge kernels meets more contacts than the queue holds."""
    for W, D, slope in ((640, 32, 0.06), (1280, 64, 0.04)):
        bands = [(40, 3, slope)]
        L, R = banded(1, W, D, bands)
        j = _job(orc, "overflow%d" % W, L, R, dict(BM, numDisparities=D, disp12MaxDiff=100, speckleRange=0), HV_WINDOWS, bands)
        j["measured"]["contacts"] = require_overflow(j["d"], j["FIL"], 0, j["vy0"], j["vy1"])
        j["measured"]["hv_boundary"] = require_hv_boundary(orc, j["d"], j["FIL"], 0, j["hv"])
        yield j


def mark_jobs(orc):
    """Case 2: three bands; short runs that survive only because a long run many rows away is in their component."""
    for bands, rng_, win in MARK_CASES:
        L, R = banded(1, 640, 32, bands)
        j = _job(orc, "marks_r%d_w%d" % (rng_, win), L, R, dict(BM, disp12MaxDiff=1, speckleRange=rng_), (win,), bands)
        j["measured"]["rescue"] = require_rescue(j["d"], j["FIL"], rng_, win)
        if win == 3:
            j["measured"]["exact"] = require_exact_sizes(j["d"], j["FIL"], rng_, win)
        yield j


def block_jobs(orc):
    """Case 3: every number of checked rows 1 .. 9 and 33, and every vy0 of 0 .. 3 above the unrestricted one."""
    for H, off in BLOCK_HEIGHTS + [(ROI_HEIGHT, o) for o in ROI_OFFSETS]:
        bands = [(H, 3, 0.06)]
        L, R = banded(1, 320, 32, bands)
        kw = dict(BM, disp12MaxDiff=100, speckleRange=0)
        if off:
            kw["roi1"] = (0, off, 320, H - off)
        j = _job(orc, "rows_h%d_o%d" % (H, off), L, R, kw, (lambda hv: hv,), bands)
        assert j["vy1"] - j["vy0"] == H - 8 - off == j["hv"], (H, off, j["vy0"], j["vy1"], j["hv"])
        j["measured"]["pairs"] = require_every_pair_in_contact(j["d"], j["FIL"], 0, j["vy0"], j["vy1"], j["hv"])
        yield j


def head_jobs(orc):
    """Case 4: the forms with one head column per pixel.  disp12MaxDiff = -1: k_spk_init + k_spk_merge_strip<4, false>, at a
    width that is and one that is not a multiple of 8; SAD sums past 16 bits (preFilterCap 63, blockSize 23): the scalar
    k_lrcheck.  The one-band inputs overflow that kernel's queue as well; the three bands carry marks through it."""
    for name, W, bands, extra, wins in (
            ("heads640", 640, ONE_BAND, dict(disp12MaxDiff=-1), HV_WINDOWS[:2]),
            ("heads644", 644, ONE_BAND, dict(disp12MaxDiff=-1), HV_WINDOWS[:2]),
            ("scalar_lr", 640, ONE_BAND, dict(disp12MaxDiff=100, preFilterCap=63, blockSize=23), HV_WINDOWS[:2]),
            ("heads_marks", 640, THREE_BANDS_03, dict(disp12MaxDiff=-1), (3,))):
        L, R = banded(1, W, 32, bands)
        j = _job(orc, name, L, R, dict(BM, speckleRange=0, **extra), wins, bands)
        if bands is ONE_BAND:
            cand = new_run_contacts(j["d"], j["FIL"], 0)
            n = max_contacts_per_workgroup(cand, pair_rows(j["vy0"], j["vy1"]))      # (strips of four pairs meet more still)
            assert n >= OVERFLOW_MIN, (name, n)
            j["measured"]["contacts"] = n
            j["measured"]["hv_boundary"] = require_hv_boundary(orc, j["d"], j["FIL"], 0, j["hv"])
        else:
            j["measured"]["rescue"] = require_rescue(j["d"], j["FIL"], 0, 3)
        yield j


def batch_jobs(orc):
    """Case 5: the four distinct pairs of the device-resident batches."""
    for seed in BATCH_SEEDS:
        L, R = banded(seed, 640, 32, ONE_BAND)
        j = _job(orc, "batch_s%d" % seed, L, R, dict(BM, disp12MaxDiff=100, speckleRange=0), (lambda hv: hv,), ONE_BAND)
        j["measured"]["contacts"] = require_overflow(j["d"], j["FIL"], 0, j["vy0"], j["vy1"])
        j["measured"]["hv_boundary"] = require_hv_boundary(orc, j["d"], j["FIL"], 0, j["hv"])
        yield j


def single_frame_jobs(orc):
    for gen in (overflow_jobs, mark_jobs, block_jobs, head_jobs):
        yield from gen(orc)


def band_spans(bands):
    y = 0
    for rows, _, _ in bands:
        yield y, y + rows
        y += rows


def interior_rows_identical(j, r):
    """the rows of a band more than r rows from its ends (the window's r rows and one more for the prefilter's 3 x 3
    kernel), inside the checked rows, all hold the same disparities"""
    r += 1
    n = 0
    for y0, y1 in band_spans(j["bands"]):
        lo = max(y0 + (r if y0 > 0 else 0), j["vy0"])
        hi = min(y1 - (r if y1 < j["d"].shape[0] else 0), j["vy1"])
        for y in range(lo + 1, hi):
            if not np.array_equal(j["d"][y], j["d"][lo]):
                return False
            n += 1
    return n > 0 or j["vy1"] - j["vy0"] == 1


# ---- StereoSGBM ----------------------------------------------------------------------------------------------------------
SGM = dict(numDisparities=32, blockSize=5, uniquenessRatio=0, disp12MaxDiff=1)
SGM_CASES = [(W, paths, rng_, win) for W in (640, 644) for paths in (8, 5) for rng_, win in ((0, 3), (1, 20))]


def sgm_frames(W, one_band=False):
    return banded(1, W, 32, ONE_BAND if one_band else THREE_BANDS_03)
