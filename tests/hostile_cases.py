"""The tables that tests/test_hostile_pairs_cpu.py and tests/test_search_plan_cpu.py verify on the CPU and that
tests/test_gpu_search_hostile.py then runs on the device.  Rows are (W, H, D, w, minD, cap, legacy) as in
test_gpu_search_routes.ROWS (whose table is repeated in test_search_plan_cpu.TABLE)."""

# The largest preFilterCap at which each row of test_gpu_search_routes.ROWS keeps its route at n = 1 AND n = 16, by the route's
# own bound (test_search_plan_cpu.test_largest_cap_of_every_route: the plan is the same there and, below 63, another one step up):
#   ROWS border form      64 w 2 cap <= 65535                      w 9: 56, w 15: 34
#   packed tile kernels   2 cap w w <= 32766                       w 17: 56, w 23: 30
#   generic_u16           2 cap w w < 65536                        w 25: 52
#   everything else       cap <= 63 (what cv::StereoBM accepts)
MAXCAP = {(300, 80, 64, 9, 0, 31, 0): 56, (560, 90, 256, 15, 0, 15, 0): 34, (250, 66, 32, 9, 0, 63, 0): 63,
          (300, 80, 64, 9, 0, 63, 0): 63, (300, 80, 80, 9, 0, 31, 0): 63, (300, 80, 64, 17, 0, 31, 0): 56,
          (200, 50, 64, 23, 0, 30, 0): 30, (300, 80, 64, 9, -7, 31, 1): 63, (300, 90, 64, 25, 0, 31, 0): 52,
          (400, 80, 272, 9, 0, 31, 0): 63}

# Boundary pairs: (parameter, family, seed, v) -- the oracle's map of hostile_pairs.make(family, seed, ...) at parameter = v
# differs from the one at v + 1 on at least 50 pixels (speckle filter off; for disp12MaxDiff also uniquenessRatio =
# textureThreshold = 0).  Found by sweeping the oracle; test_hostile_pairs_cpu.test_pinned_boundaries_are_live keeps them honest.
# textureThreshold is live at multiples of cap (of w cap where the bars run through the window), uniquenessRatio where
# minsad (100 + v) / 100 crosses a small multiple of cap.
TEX, UNIQ, D12 = "textureThreshold", "uniquenessRatio", "disp12MaxDiff"
PINS = {
    (300, 80, 64, 9, 0, 31, 0): [(TEX, "bars", 2, 279), (TEX, "bars", 2, 1116), (UNIQ, "bars", 0, 0), (UNIQ, "steps", 1, 7), (D12, "steps", 8, 0), (D12, "steps", 4, 1)],
    (300, 80, 64, 9, 0, 56, 0): [(TEX, "bars", 2, 504), (TEX, "bars", 2, 2016), (UNIQ, "bars", 0, 0), (UNIQ, "steps", 0, 7), (D12, "steps", 8, 0), (D12, "steps", 8, 1)],
    (560, 90, 256, 15, 0, 15, 0): [(TEX, "bars", 2, 225), (TEX, "bars", 2, 900), (UNIQ, "bars", 1, 0), (UNIQ, "steps", 1, 33), (D12, "steps", 8, 0), (D12, "steps", 5, 1)],
    (560, 90, 256, 15, 0, 34, 0): [(TEX, "bars", 2, 510), (TEX, "bars", 2, 2040), (UNIQ, "bars", 1, 0), (UNIQ, "steps", 2, 24), (D12, "steps", 8, 0), (D12, "steps", 5, 1)],
    (250, 66, 32, 9, 0, 63, 0): [(TEX, "bars", 1, 567), (TEX, "bars", 2, 2268), (UNIQ, "plateau_noise", 1, 0), (UNIQ, "bars", 1, 99), (D12, "steps", 7, 0), (D12, "steps", 8, 1)],
    (300, 80, 64, 9, 0, 63, 0): [(TEX, "bars", 2, 567), (TEX, "bars", 2, 2268), (UNIQ, "bars", 0, 0), (UNIQ, "steps", 0, 7), (D12, "steps", 8, 0), (D12, "steps", 4, 1)],
    (300, 80, 80, 9, 0, 31, 0): [(TEX, "bars", 2, 279), (TEX, "bars", 2, 1116), (UNIQ, "bars", 1, 0), (UNIQ, "steps", 1, 7), (D12, "steps", 6, 0), (D12, "steps", 11, 1)],
    (300, 80, 80, 9, 0, 63, 0): [(TEX, "bars", 2, 567), (TEX, "bars", 2, 2268), (UNIQ, "bars", 1, 0), (UNIQ, "steps", 1, 7), (D12, "steps", 3, 0), (D12, "steps", 4, 1)],
    (300, 80, 64, 17, 0, 31, 0): [(TEX, "bars", 1, 527), (TEX, "bars", 1, 2108), (UNIQ, "plateau_noise", 1, 0), (UNIQ, "plateau_noise", 1, 7), (D12, "steps", 13, 0), (D12, "steps", 15, 1)],
    (300, 80, 64, 17, 0, 56, 0): [(TEX, "bars", 1, 952), (TEX, "bars", 1, 3808), (UNIQ, "plateau_noise", 1, 0), (UNIQ, "steps", 0, 42), (D12, "steps", 13, 0), (D12, "steps", 6, 1)],
    (200, 50, 64, 23, 0, 30, 0): [(TEX, "bars", 2, 480), (TEX, "bars", 1, 840), (UNIQ, "plateau_noise", 1, 0), (UNIQ, "steps", 0, 49), (D12, "steps", 5, 0), (D12, "steps", 6, 1)],
    (300, 80, 64, 9, -7, 31, 1): [(TEX, "bars", 2, 279), (TEX, "bars", 2, 1116), (UNIQ, "bars", 1, 0), (UNIQ, "plateau_noise", 1, 7), (D12, "steps", 8, 0), (D12, "steps", 3, 1)],
    (300, 80, 64, 9, -7, 63, 1): [(TEX, "bars", 2, 567), (TEX, "bars", 2, 2268), (UNIQ, "bars", 1, 0), (UNIQ, "plateau_noise", 1, 7), (D12, "steps", 8, 0), (D12, "steps", 6, 1)],
    (300, 90, 64, 25, 0, 31, 0): [(TEX, "bars", 1, 775), (TEX, "bars", 1, 3100), (UNIQ, "plateau_noise", 2, 0), (UNIQ, "steps", 1, 42), (D12, "steps", 5, 0), (D12, "steps", 4, 1)],
    (300, 90, 64, 25, 0, 52, 0): [(TEX, "bars", 1, 1300), (TEX, "bars", 1, 5200), (UNIQ, "plateau_noise", 2, 0), (UNIQ, "steps", 1, 42), (D12, "steps", 5, 0), (D12, "steps", 11, 1)],
    (400, 80, 272, 9, 0, 31, 0): [(TEX, "bars", 2, 279), (TEX, "bars", 1, 1116), (UNIQ, "bars", 0, 0), (UNIQ, "steps", 1, 7), (D12, "steps", 4, 0), (D12, "bars", 15, 1)],
    (400, 80, 272, 9, 0, 63, 0): [(TEX, "bars", 2, 567), (TEX, "bars", 1, 2268), (UNIQ, "bars", 0, 0), (UNIQ, "steps", 1, 7), (D12, "steps", 4, 0), (D12, "bars", 15, 1)],
}
# Border kernels at their bounds, frames of at least 64 + w + 8 rows (test_search_plan_cpu pins the border form of either):
#   ROWS (k_search_border2): 64-row packed prefix sums, 64 w 2 cap = 65280 at w 15, cap 34 (blockSize is odd: no w 16)
#   DISP (k_search_border) at its widest window, w 21, at the largest cap the tile kernel beside it takes: 2 cap w w = 32634 at
#   cap 37.  (plan_border would let DISP run up to 2 cap w w <= 65535, but no packed tile kernel exists above 32766, and
#   without one the generic kernel takes the border columns as well: that half of DISP's range cannot be reached.)
BORDER_ROWS_ROW = (300, 88, 64, 15, 0, 34, 0)
BORDER_DISP_ROW = (300, 94, 64, 21, 0, 37, 0)
SPECKLE_OFF = dict(speckleWindowSize=0)


def pin_params(name, v):
    """The oracle's / the matcher's keyword parameters of a pinned boundary at value v."""
    kw = dict(SPECKLE_OFF)
    if name == D12:
        kw.update(uniquenessRatio=0, textureThreshold=0)
    kw[name] = v
    return kw


def with_cap(row, cap):
    return row[:5] + (cap,) + row[6:7]


# Batches whose strips walk more rows than two rebase intervals of the ring: (frames, row, lanes per pixel).  One
# instantiation per lanes-per-pixel value, at the largest cap that still rebases (w 15: cap 59 -- 65535 / (15 * 118) - 21 = 16
# rows, one trip of 16; w 13, two lanes: cap 63 -- 21 rows, one trip of 14).  test_search_plan_cpu pins the strips.
LONG_STRIPS = [(2048, (85, 52, 32, 13, 0, 63, 0), 2), (512, (119, 54, 64, 15, 0, 59, 0), 4),
               (512, (183, 54, 128, 15, 0, 59, 0), 8), (512, (301, 54, 256, 15, 0, 59, 0), 16)]
# The forms that do NOT rebase (one trip of the row loop is longer than ring_rows_cap: w 15 at cap 63, 13 rows; w 13 with four
# rows per group at cap 63, 21 rows) live on ring_min_strips alone.  Frames of exactly three full strips, 3 x ring_rows_cap
# output rows, in batches large enough that the model stays at that minimum (w 13: a single frame would be cut into four
# strips of 16): every strip has the full allowed length.  test_search_plan_cpu pins rows_per_strip == ring_rows_cap.
NO_REBASE_STRIPS = [(16, (107, 53, 32, 15, 0, 63, 0), 2), (16, (139, 53, 64, 15, 0, 63, 0), 4), (16, (203, 53, 128, 15, 0, 63, 0), 8),
                    (16, (267, 53, 192, 15, 0, 63, 0), 8), (16, (331, 53, 256, 15, 0, 63, 0), 16),
                    (512, (137, 75, 64, 13, 0, 63, 0), 4), (512, (169, 75, 96, 13, 0, 63, 0), 4), (256, (201, 75, 128, 13, 0, 63, 0), 8),
                    (256, (265, 75, 192, 13, 0, 63, 0), 8), (256, (329, 75, 256, 13, 0, 63, 0), 16)]
# the shape of test_gpu_ring_pair.test_strips_longer_than_the_rebase_interval at cap 63 (at cap 31 its strips cross one rebase)
LONG_STRIPS_64_9_4 = [(8192, (128, 200, 64, 9, 0, 63, 0), 4)]


def ring_rows_cap(w, cap):
    """Rows a strip may have so that no packed prefix sum leaves 16 bits (k_search_ring.hip)."""
    return 65535 // (w * 2 * cap) - w - 6


def ring_trip(D, w, lpp):
    W1, rpg = w + 1, (4 if D >= 96 else lpp)
    return W1 if W1 % rpg == 0 else 2 * W1 if 2 * W1 % rpg == 0 else 4 * W1


def ring_rebase_trips(D, w, lpp, cap):
    return ring_rows_cap(w, cap) // ring_trip(D, w, lpp)


def largest_ring_cap(w):
    """The largest cap below 64 that keeps a ring form: 2 cap w w < 0x7C00 (and a strip of at least two rows)."""
    return max(c for c in range(1, 64) if 2 * c * w * w < 0x7C00 and ring_rows_cap(w, c) >= 2)
