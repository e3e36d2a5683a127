"""The compact-head speckle merge settles a (chunk, row pair) item from the two head records and one run-list entry each,
without reading the disparities (tests/settled.py restates the record format, the classification and the rule).  On random
run layouts: (a) a settled pair holds no contact, or only contacts between two runs that are both longer than the window,
by the plain definition from the disparities; (b) the unions and marks the kernel's rules produce -- with the left-neighbour
bit reading 0 behind a settled neighbour, with contacts on the overflow path, in any order -- filter the map exactly as
oracle.filter_speckles does."""
import numpy as np
import pytest

import settled as S

FIL = -16
WINDOWS = (7, 8, 9, 16, 100)
WIDTHS = (61, 64, 100, 203, 636)              # 636 % 8 == 4: a ragged last chunk; 636 > 512: a second wave in a row


def random_map(rng, W, H, win, maxDiff):
    """Rows of runs with lengths around the window, short ones, and long ones that end wherever they end (mid-chunk as a
    rule), gaps of invalid pixels, whole invalid rows.  Adjacent runs differ by more than maxDiff; the same few levels on
    every row, so runs of neighbouring rows touch."""
    levels = 160 + np.arange(5) * (maxDiff + 9)
    d = np.full((H, W), FIL, np.int64)
    for y in range(H):
        if rng.random() < 0.12:
            continue                                          # a row without a valid pixel
        x, last = 0, -1
        if y and rng.random() < 0.4:                         # mostly the row above, shifted: long runs over long runs
            sh = int(rng.integers(-3, 4))
            d[y] = np.roll(d[y - 1], sh)
            if sh > 0: d[y, :sh] = FIL
            if sh < 0: d[y, sh:] = FIL
            continue
        while x < W:
            kind = rng.random()
            if kind < 0.25:
                x += int(rng.integers(1, 20))                 # invalid pixels
                last = -1
                continue
            if kind < 0.55:
                ln = win + int(rng.integers(-1, 2))           # window - 1, window, window + 1
            elif kind < 0.75:
                ln = int(rng.integers(1, 5))
            else:
                ln = int(rng.integers(win + 1, 4 * win + 40))
            lv = int(rng.integers(0, len(levels)))
            if lv == last:
                lv = (lv + 1) % len(levels)
            last = lv
            ln = min(ln, W - x)
            jit = rng.integers(0, maxDiff // 2 + 1, ln)       # inside a run neighbours stay within maxDiff
            d[y, x:x + ln] = levels[lv] + jit
            x += ln
    return d.astype(np.int16)


def cases():
    for i, W in enumerate(WIDTHS):
        for j, win in enumerate(WINDOWS):
            yield W, win, (0, 32)[(i + j) % 2], 1000 * i + j


@pytest.fixture(scope="module")
def maps():
    out = {}
    for W, win, md, seed in cases():
        rng = np.random.default_rng(seed)
        out[(W, win)] = (random_map(rng, W, 14 if W > 300 else 24, win, md), md)
    return out


def test_the_records_rebuild_every_pixels_run(maps):
    # node of the pixel at bit k = cnt + popcount(starts at or left of k) - 1, and the run list entry of that node covers it
    for (W, win), (d, md) in maps.items():
        v, start, runs = S.row_tables(d, FIL, md)
        cnt, starts = S.records(start)
        for y in range(d.shape[0]):
            for x in np.flatnonzero(v[y]):
                c, k = divmod(int(x), 8)
                i = int(cnt[y, c]) + bin(int(starts[y, c]) & ((2 << k) - 1)).count("1") - 1
                rx, ln = runs[y][i]
                assert rx <= x < rx + ln, (W, win, y, x)


def test_the_inputs_hold_every_class_and_both_kinds_of_pair(maps):
    seen, ended_at, long_end_at = set(), set(), set()
    ns = nu = 0
    for (W, win), (d, md) in maps.items():
        cls = S.classes(d, FIL, md, win)
        seen |= set(np.unique(cls))
        s, u = S.item_mix(d, FIL, md, win)
        ns += s; nu += u
        _, start, runs = S.row_tables(d, FIL, md)
        cnt, starts = S.records(start)
        # a chunk with runs left of it whose last run ended before the chunk, and a long run that ends inside a chunk
        ended = [(y, c) for y in range(d.shape[0]) for c in range(cnt.shape[1])
                 if starts[y, c] == 0 and cnt[y, c] > 0 and sum(runs[y][cnt[y, c] - 1]) <= 8 * c]
        if ended:
            ended_at.add(win)
        if any(ln > win and (x + ln) % 8 and x + ln < W and d[y, x + ln] == FIL for y, row in enumerate(runs) for x, ln in row):
            long_end_at.add(win)                              # ... followed by invalid pixels
    assert seen == {S.EMPTY, S.LONG, S.UNDECIDED}
    assert ns >= 0.25 * (ns + nu) and nu >= 0.05 * (ns + nu), (ns, nu)
    assert ended_at == set(WINDOWS) and long_end_at == set(WINDOWS), (ended_at, long_end_at)
    lens = {ln for (W, win), (d, md) in maps.items() if win == 8 for row in S.row_tables(d, FIL, md)[2] for _, ln in row}
    assert {7, 8, 9} <= lens


def test_every_contact_of_a_settled_pair_is_long_long(maps):
    nsettled_with_contact = 0
    for (W, win), (d, md) in maps.items():
        settled = S.settled_pairs(S.classes(d, FIL, md, win))
        contact, longlong = S.contact_kinds(d, FIL, md, win)
        per_px = np.repeat(settled, 8, axis=1)[:, :W]
        assert not (per_px & contact & ~longlong).any(), (W, win)
        nsettled_with_contact += int((per_px & contact).any(axis=0).sum())
    assert nsettled_with_contact > 100                        # (the rule is not vacuous: settled pairs do carry contacts)


@pytest.mark.parametrize("leftc,overflow", [("wave", 0.0), ("lane", 0.0), ("memory", 0.0), ("lane", 0.3), ("wave", 1.0)])
def test_the_kernels_rules_filter_like_the_oracle(maps, oracle, leftc, overflow):
    nq_lane = nq_memory = 0
    for n, ((W, win), (d, md)) in enumerate(maps.items()):
        want = oracle.filter_speckles(d, FIL, win, md)
        got, nq = S.kernel_filter(d, FIL, md, win, leftc=leftc, overflow=overflow, rng=np.random.default_rng(n), wave0=8 * n)
        assert np.array_equal(got, want), (W, win, md, int((got != want).sum()))
        assert (want != d).any() and (want != FIL).any(), (W, win)
        if leftc == "wave" and overflow == 0.0:               # the model without the rule: the kernel as it was
            base, _ = S.kernel_filter(d, FIL, md, win, leftc=leftc, skip=False, rng=np.random.default_rng(n), wave0=8 * n)
            assert np.array_equal(base, want), (W, win)
        if leftc == "lane" and overflow == 0.0:
            nq_lane += nq
            nq_memory += S.kernel_filter(d, FIL, md, win, leftc="memory")[1]
    if leftc == "lane" and overflow == 0.0:
        assert nq_lane > nq_memory                            # duplicates behind settled neighbours were queued, and dropped


def test_a_duplicate_behind_a_settled_neighbour_is_long_long():
    # two long runs, one over the other, across chunks 0..3; the lower row's chunk 2 starts a short run at its first
    # pixel, so chunk 2 is unsettled next to the settled chunk 1 and its lane-fed left bit reads 0
    W, win = 40, 8
    d = np.full((4, W), FIL, np.int16)
    d[1, 0:30] = 200
    d[2, 0:16] = 200
    d[2, 16:19] = 300                                        # the short run at the first pixel of chunk 2
    d[2, 19:34] = 200
    cls = S.classes(d, FIL, 0, win)
    assert cls[1, 1] == S.LONG and cls[2, 1] == S.LONG and cls[2, 2] == S.UNDECIDED and cls[1, 2] == S.LONG
    s = S.settled_pairs(cls)
    assert s[1, 1] and not s[1, 2]
    from oracle import oracle as orc
    orc.build()
    want = orc.filter_speckles(d, FIL, win, 0)
    for leftc in ("lane", "memory"):
        got, _ = S.kernel_filter(d, FIL, 0, win, leftc=leftc)
        assert np.array_equal(got, want), leftc
    assert (want[2, 16:19] == FIL).all() and (want[2, 19:34] == 200).all()


def test_the_gpu_tests_inputs_hold_their_cases(oracle):
    # tests/test_gpu_speckle_settled.py asserts the same before it looks at a device result; here an input that drifts fails
    # on a machine without a GPU first
    total = S.require_cases(list(S.jobs(oracle)))
    assert len(total) == len(S.WIDTHS) * 2 * len(S.WINDOWS)
