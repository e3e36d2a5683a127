"""A numpy restatement of what the compact-head speckle merge (k_spk_merge_strip<RS, true>) reads and decides: the head
record of an 8-column chunk, the row's dense run list, the classification of a chunk-row from those two alone, the
"settled pair" rule that lets the kernel skip the disparity rows, and the unions and marks that follow.  A helper: no
test in here, nothing imported from the kernels.

Record of chunk c of a row: cnt | starts << 16 -- cnt = runs of the row that start left of column 8 c, starts bit k = a run
starts at column 8 c + k.  Run list of a row: (x, len) per run, in order.  The node of a run is (row, index in the row).
"""
import numpy as np

EMPTY, LONG, UNDECIDED = 0, 1, 2


def row_tables(d, FIL, maxDiff):
    """-> valid [H, W], start [H, W] (the pixel starts a horizontal run), runs: per row a list of (x, len)."""
    d = np.asarray(d).astype(np.int64)
    v = d != FIL
    start = v.copy()
    start[:, 1:] &= ~(v[:, 1:] & v[:, :-1] & (np.abs(d[:, 1:] - d[:, :-1]) <= maxDiff))
    runs = []
    for y in range(d.shape[0]):
        xs = np.flatnonzero(start[y])
        row = []
        for x in xs:
            e = x + 1
            while e < d.shape[1] and v[y, e] and not start[y, e]:
                e += 1
            row.append((int(x), int(e - x)))
        runs.append(row)
    return v, start, runs


def records(start):
    """-> cnt [H, nxb], starts [H, nxb]: the two fields of every chunk's head record."""
    H, W = start.shape
    nxb = (W + 7) // 8
    s = np.zeros((H, nxb * 8), np.int64)
    s[:, :W] = start
    s = s.reshape(H, nxb, 8)
    per = s.sum(axis=2)
    cnt = np.cumsum(per, axis=1) - per
    starts = (s << np.arange(8)).sum(axis=2)
    return cnt, starts


def classify(cnt, starts, row_runs, x0, maxSize):
    """What the kernel knows of a chunk-row before it reads a disparity."""
    if starts != 0:
        return UNDECIDED
    if cnt == 0:
        return EMPTY
    x, ln = row_runs[cnt - 1]                          # the one look-up
    if x + ln <= x0:
        return EMPTY
    return LONG if ln > maxSize else UNDECIDED


def classes(d, FIL, maxDiff, maxSize, tables=None):
    """-> [H, nxb] array of EMPTY / LONG / UNDECIDED.  tables: row_tables(d, FIL, maxDiff), if at hand."""
    _, start, runs = tables or row_tables(d, FIL, maxDiff)
    cnt, starts = records(start)
    H, nxb = cnt.shape
    return np.array([[classify(int(cnt[y, c]), int(starts[y, c]), runs[y], 8 * c, maxSize) for c in range(nxb)] for y in range(H)])


def settled_pairs(cls):
    """[H - 1, nxb] bool: the pair (y, y + 1) of a chunk needs no disparity"""
    a, b = cls[:-1], cls[1:]
    return (a == EMPTY) | (b == EMPTY) | ((a == LONG) & (b == LONG))


def _find(parent, x):
    while parent[x] != x:
        parent[x] = parent[parent[x]]
        x = parent[x]
    return x


def _union(parent, a, b):
    a, b = _find(parent, a), _find(parent, b)
    if a != b:
        parent[max(a, b)] = min(a, b)


def kernel_filter(d, FIL, maxDiff, maxSize, leftc="wave", skip=True, overflow=0.0, rng=None, wave0=0):
    """The filtered map from the kernel's rules.  leftc: where the contact bit of the pixel left of a chunk comes from --
    "lane": always the left neighbour's mask (0 if its pair was settled), "memory": always the disparities, "wave": from the
    disparities for every 64th thread (threads numbered row-major over the pairs, from wave0), else from the neighbour.
    skip = False: nothing is settled (the kernel before the change).  overflow: the share of contacts that take the queue
    overflow path (a plain union, no large-run shortcut).  Contacts are dealt with in a random order.
    -> (map, number of queued contacts)"""
    rng = rng or np.random.default_rng(0)
    d = np.asarray(d).astype(np.int64)
    H, W = d.shape
    v, start, runs = row_tables(d, FIL, maxDiff)
    cnt, starts = records(start)
    nxb = cnt.shape[1]
    cls = classes(d, FIL, maxDiff, maxSize)
    settled = settled_pairs(cls) if skip else np.zeros((H - 1, nxb), bool)
    ev = np.zeros((H - 1, nxb * 8), bool)
    ev[:, :W] = v[1:] & v[:-1] & (np.abs(d[1:] - d[:-1]) <= maxDiff)
    contacts = []
    for y in range(H - 1):
        prev_cm = 0
        for c in range(nxb):
            cm = 0 if settled[y, c] else int((ev[y, 8 * c:8 * c + 8] << np.arange(8)).sum())
            thread = wave0 + y * nxb + c
            if c == 0:
                lc = 0
            elif leftc == "memory" or (leftc == "wave" and thread % 64 == 0):
                lc = int(ev[y, 8 * c - 1]) if cm else 0
            else:
                lc = prev_cm >> 7
            sa, sb = int(starts[y, c]), int(starts[y + 1, c])
            cand = cm & ~(((cm << 1) | lc) & ~sa & ~sb) & 0xff
            for k in range(8):
                if (cand >> k) & 1:
                    m = (2 << k) - 1
                    na = int(cnt[y, c]) + bin(sa & m).count("1") - 1
                    nb = int(cnt[y + 1, c]) + bin(sb & m).count("1") - 1
                    contacts.append(((y, na), (y + 1, nb)))
            prev_cm = cm
    node = {}
    for y in range(H):
        for i in range(len(runs[y])):
            node[(y, i)] = len(node)
    size = np.array([ln for row in runs for _, ln in row], np.int64)
    parent = list(range(len(node)))
    for i in rng.permutation(len(contacts)):
        a, b = node[contacts[i][0]], node[contacts[i][1]]
        if rng.random() < overflow:
            _union(parent, a, b)
            continue
        la, lb = size[a] > maxSize, size[b] > maxSize       # uf_union_contact
        if la or lb:
            if la != lb:
                size[b if la else a] = max(size[b if la else a], maxSize + 1)
            continue
        _union(parent, a, b)
    for i in range(len(node)):                               # k_spk_count
        r = _find(parent, i)
        if r != i and size[r] <= maxSize:
            size[r] += size[i]
    out = np.array(d, np.int16, copy=True)                   # k_spk_apply
    for y in range(H):
        for i, (x, ln) in enumerate(runs[y]):
            if ln <= maxSize and size[_find(parent, node[(y, i)])] <= maxSize:
                out[y, x:x + ln] = FIL
    return out, len(contacts)


def run_length_map(d, FIL, maxDiff, tables=None):
    """Per pixel: the length of its horizontal run (0 where invalid), from the disparities alone."""
    v, _, runs = tables or row_tables(d, FIL, maxDiff)
    ln = np.zeros(v.shape, np.int64)
    for y, row in enumerate(runs):
        for x, n in row:
            ln[y, x:x + n] = n
    return ln


def contact_kinds(d, FIL, maxDiff, maxSize):
    """-> (contact [H - 1, W]: (y, x) touches (y + 1, x); longlong [H - 1, W]: both pixels lie in runs longer than maxSize)"""
    d = np.asarray(d).astype(np.int64)
    v = d != FIL
    ln = run_length_map(d, FIL, maxDiff)
    contact = v[1:] & v[:-1] & (np.abs(d[1:] - d[:-1]) <= maxDiff)
    return contact, (ln[1:] > maxSize) & (ln[:-1] > maxSize)


def item_mix(d, FIL, maxDiff, maxSize, y0=0, y1=None):
    """-> (settled, unsettled) numbers of (chunk, row pair) items of the rows [y0, y1)"""
    s = settled_pairs(classes(np.asarray(d)[y0:y1], FIL, maxDiff, maxSize))
    return int(s.sum()), int((~s).sum())


# ---- the inputs of tests/test_gpu_speckle_settled.py: extruded bands (tests/extruded.py) with flat column zones --------
# A flat zone has no texture, so with textureThreshold > 0 the matcher leaves it invalid: whole chunks without a valid pixel
# (settled as "empty"), runs that end inside a chunk with invalid pixels behind them, and textured zones whose width sets
# the length of the run they carry (a clean zone of T columns carries a run of T - 1: 101 and 102 columns for runs of
# exactly 100 and 101).  The middle band is textured across the zones of its neighbours: long runs over short ones.
H_ROWS = 40
BANDS = [(14, 3, 0.0), (12, 3, 0.0), (14, 3, 0.0)]
ZONES = [[(40, 101), (165, 102), (290, 101), (415, 102), (540, 60)],
         [(40, 420)],
         [(28, 102), (160, 101), (290, 60)]]
KW = dict(numDisparities=32, blockSize=9, uniquenessRatio=0, textureThreshold=10, disp12MaxDiff=100)
WINDOWS = (7, 8, 9, 15, 16, 17, 100)
WIDTHS = (640, 636)
SEEDS = (3, 5, 6, 10)                                 # a batch cycles four distinct pairs


def frames(W, seed):
    """-> contiguous uint8 (L, R), H_ROWS x W"""
    import extruded as E
    L, R = E.banded(seed, W, 32, BANDS)
    y = 0
    for (rows, _, _), zones in zip(BANDS, ZONES):
        keep = np.zeros(W, bool)
        for x, w in zones:
            keep[x:x + w] = True
        L[y:y + rows, ~keep] = 128
        R[y:y + rows, ~keep] = 128
        y += rows
    return L, R


def cases_present(d, FIL, maxDiff, maxSize, vy0, vy1, tables=None):
    """How often each situation the merge kernel must get right occurs in rows [vy0, vy1) of the unfiltered map d.
    tables: row_tables(d[vy0:vy1], FIL, maxDiff), if at hand."""
    d = np.asarray(d)[vy0:vy1].astype(np.int64)
    H, W = d.shape
    tables = tables or row_tables(d, FIL, maxDiff)
    v, start, runs = tables
    cnt, starts = records(start)
    cls = classes(d, FIL, maxDiff, maxSize, tables)
    st = settled_pairs(cls)
    ln = run_length_map(d, FIL, maxDiff, tables)
    contact = v[1:] & v[:-1] & (np.abs(d[1:] - d[:-1]) <= maxDiff)
    nxb = cnt.shape[1]
    out = dict(settled=int(st.sum()), unsettled=int((~st).sum()))
    # a long run whose end falls inside a chunk, followed by invalid pixels
    out["long_end_mid_chunk"] = sum(1 for y, row in enumerate(runs) for x, n in row
                                    if n > maxSize and (x + n) % 8 and x + n < W and not v[y, x + n])
    # a chunk with runs left of it whose last run ended in an earlier chunk
    out["ended_before_chunk"] = sum(1 for y in range(H) for c in range(nxb)
                                    if starts[y, c] == 0 and cnt[y, c] > 0 and sum(runs[y][cnt[y, c] - 1]) <= 8 * c)
    # a long run in contact with a run of exactly the window length / one more
    a, b = ln[:-1], ln[1:]
    out["long_on_exact"] = int((contact & (((a > maxSize) & (b == maxSize)) | ((b > maxSize) & (a == maxSize)))).sum())
    out["runs_exact"] = sum(1 for row in runs for _, n in row if n == maxSize)
    out["runs_one_more"] = sum(1 for row in runs for _, n in row if n == maxSize + 1)
    # a long-long pair whose right neighbour chunk starts a short run at its first pixel
    n = 0
    for y in range(H - 1):
        for c in range(nxb - 1):
            if cls[y, c] == LONG and cls[y + 1, c] == LONG:
                for yy in (y, y + 1):
                    if starts[yy, c + 1] & 1 and 0 < ln[yy, 8 * c + 8] <= maxSize:
                        n += 1
    out["short_start_right_of_long_long"] = n
    # an unsettled chunk at x0 = 512 (the first lane of a wave in every fourth strip of a 640-wide frame) beside a settled one
    out["wave_start_beside_settled"] = int((~st[:, 64] & st[:, 63]).sum()) if nxb > 64 else 0
    out["settled_with_contact"] = int((np.repeat(st, 8, axis=1)[:, :W] & contact).sum())
    return out


RANGE_CASES = ("long_end_mid_chunk", "ended_before_chunk", "long_on_exact", "runs_exact", "runs_one_more",
               "short_start_right_of_long_long", "wave_start_beside_settled", "settled_with_contact")


def jobs(orc):
    """Every (width, pair, speckleRange, window) the GPU test runs, with the oracle's unfiltered map and what it holds."""
    import extruded as E
    for W in WIDTHS:
        for seed in SEEDS:
            L, R = frames(W, seed)
            for rng_ in (0, 32):
                kw = dict(KW, speckleRange=rng_)
                d = E.unfiltered(orc, L, R, **kw)
                vy0, vy1 = E.checked_rows(orc, L, kw)
                tables = row_tables(d[vy0:vy1], E.fil(kw), rng_)
                for win in WINDOWS:
                    yield dict(W=W, seed=seed, rng=rng_, win=win, L=L, R=R, kw=dict(kw, speckleWindowSize=win), d=d, FIL=E.fil(kw),
                               cases=cases_present(d, E.fil(kw), rng_, win, vy0, vy1, tables))


def require_cases(all_jobs):
    """Every input settles at least 25 % of its (chunk, row pair) items and leaves at least 5 % unsettled.  With
    speckleRange 32 the pairs of every width and window hold every situation of RANGE_CASES between them.  With speckleRange
    0 a run is a stretch of equal 1/16-pixel disparities, a handful of pixels: what settles there are the chunks without
    a valid pixel, found empty by the record alone or by the look-up of a run that ended before the chunk."""
    total = {}
    for j in all_jobs:
        c = j["cases"]
        n = c["settled"] + c["unsettled"]
        assert c["settled"] >= 0.25 * n and c["unsettled"] >= 0.05 * n, (j["W"], j["seed"], j["rng"], j["win"], c)
        t = total.setdefault((j["W"], j["rng"], j["win"]), dict.fromkeys(RANGE_CASES, 0))
        for k in RANGE_CASES:
            t[k] += c[k]
    for (W, rng_, win), t in total.items():
        need = RANGE_CASES if rng_ == 32 else ("ended_before_chunk",)
        assert all(t[k] >= 1 for k in need), (W, rng_, win, t)
    return total
