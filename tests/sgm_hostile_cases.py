"""What the hostile StereoSGBM suite runs: shapes, the parameter set each family of tests/sgm_hostile.py is meant for, the seeds
at which the oracle meets the conditions of tests/test_sgm_hostile_cpu.py, and the uniqueness pins.  No device, no oracle.

The seeds and pins were found by scanning seeds upwards on the oracle and are re-checked by test_sgm_hostile_cpu.py; the shares
in the comments were measured there (frame `seed`, MODE_HH / MODE_SGBM / MODE_HH4)."""

MODES = (8, 5, 4)                                   # paths: MODE_HH, MODE_SGBM, MODE_HH4
DOMAIN = (61, 23)                                   # W1, H: the cost domain of every shape (tests/test_gpu_sgm_routes.py's narrow one; the
                                                    # 20 x 12 of its wide rows holds too few pixels for the conditions to be met)
NARROW_D = (64, 128, 256, 48, 80)                   # 2, 4, 8 disparities per lane; 48 and 80 leave dead lanes
WIDE_D = (272, 1040)                                # wide_w1, wide_w4
ALL_D = NARROW_D + WIDE_D


def shape(D):
    """-> (W1, H)"""
    return DOMAIN


def width(D, minD, W1):
    return W1 + max(minD + D, 0) - min(minD, 0)


# ---- parameter sets: family -> paths -> [keyword sets of the oracle / the matcher] ------------------------------------------------
# partial_sat: fewer paths need larger penalties for the sum to reach 32767.  Measured at D = 64, blockSize 9 (share of domain
# pixels with some but not all costs saturated / of interior winners with a saturated neighbour / of pixels with every cost
# saturated / of the frame that is valid; 0.488 of the frame is domain):
#   MODE_HH   P1 5000 P2 6000    0.97 - 0.99 / 0.96 - 0.98 / 0.005 - 0.026 / 0.43 - 0.44
#   MODE_SGBM P1 8000 P2 9500    0.87 - 0.91 / 0.65 - 0.77 / 0 / 0.48
#   MODE_HH4  P1 9000 P2 11000   0.95 - 0.99 / 0.45 - 0.59 / 0 / 0.46 - 0.49
# (at blockSize 5 the block costs stay below 1000 and the lines of 61 columns and 23 rows are too short for anything to saturate)
PARTIAL_SAT = {8: dict(blockSize=9, P1=5000, P2=6000), 5: dict(blockSize=9, P1=8000, P2=9500), 4: dict(blockSize=9, P1=9000, P2=11000)}
# The second set of partial_sat: uniquenessRatio 0 and larger penalties.  Where EVERY cost of a pixel is 32767 there is no winner
# (R6: the search for a cost below SHRT_MAX finds none); at uniquenessRatio > 0 the uniqueness test rejects such a pixel anyway,
# at 0 only that rule does.  MODE_HH has 53 / 49 / 26 such pixels in the frames of D = 64 (five or four paths never get there
# on this content: tests/test_gpu_sgm_hh4.py builds its own frame for that).
PARTIAL_SAT_U0 = {8: dict(blockSize=9, P1=9000, P2=10000, uniquenessRatio=0), 5: dict(blockSize=9, P1=12000, P2=14000, uniquenessRatio=0),
                  4: dict(blockSize=9, P1=14000, P2=16000, uniquenessRatio=0)}
# at_limit: P2 = sgm_hostile_ref.limit_P2(frames) (None here), P1 = 3 P2 / 4: penalties so large that L_r = C + P2 wherever the
# previous pixel's minimum sits elsewhere -- 32767 exactly at the largest block cost.  blockSize 9: the largest block cost is
# about 2700, P2 about 30000 (rtdm_sgm_create takes P2 <= 32000).
AT_LIMIT = dict(blockSize=9, P1=None, P2=None)
# ties: uniquenessRatio 0 (at 10 every tied pixel is rejected: the map would be empty)
TIES = [dict(blockSize=1, uniquenessRatio=0), dict(blockSize=5, uniquenessRatio=0)]
# vote_ties: two grey levels, blockSize 1, the smallest penalties: minS takes few values.  uniquenessRatio 0 and no speckle
# filter: two-level content is ambiguous, at 10 / 100 the maps of the larger D are empty.  Measured at D = 64, minD 0, 3, -5:
# 27 - 42 tied votes per frame in MODE_HH, 55 - 67 in MODE_SGBM, 50 - 64 in MODE_HH4; resolving them the other way changes 33 - 90
# pixels of the raw map.
VOTE_TIES = dict(blockSize=1, P1=2, P2=5, uniquenessRatio=0, speckleWindowSize=0)
# ends: no speckle filter (its bands of two rows are smaller than the window)
ENDS = dict(blockSize=3, speckleWindowSize=0)
STEPS = dict(blockSize=5, speckleWindowSize=0)


def param_sets(family, paths):
    if family == "partial_sat":
        return [dict(PARTIAL_SAT[paths]), dict(PARTIAL_SAT_U0[paths])]
    if family in ("ties", "ties35"):
        return [dict(k) for k in TIES]
    return [dict({"at_limit": AT_LIMIT, "vote_ties": VOTE_TIES, "ends": ENDS, "steps": STEPS}[family])]


# ---- seeds: family -> D -> seed (frames seed, seed + 1, seed + 2 all meet the conditions at that D; the first that does) ---------
SEEDS = {
    "partial_sat": {272: 1001},
    "at_limit": {},
    "ties": {},
    # (where the first minimum falls against the lane rows depends on the shifts the seed draws)
    "ties35": {128: 1302, 256: 1328, 272: 1306, 1040: 1303},
    "vote_ties": {1040: 1406},
    "ends": {},
    "steps": {256: 1601},
}
FIRST_SEED = {"partial_sat": 1000, "at_limit": 1100, "ties": 1200, "ties35": 1300, "vote_ties": 1400, "ends": 1500, "steps": 1600}


def seed(family, D):
    """(test_sgm_hostile_cpu.py checks the conditions at every D of ALL_D)"""
    return SEEDS[family].get(D, FIRST_SEED[family])


# ---- uniqueness pins: (family, D, paths, seed, u): the oracle's maps at uniquenessRatio u and u + 1 differ -------------------------
PINS = [
    ("partial_sat", 64, 8, 1000, 6), ("vote_ties", 64, 5, 1400, 7), ("partial_sat", 64, 4, 1000, 8),
    ("vote_ties", 128, 8, 1400, 9), ("partial_sat", 128, 5, 1000, 10), ("vote_ties", 128, 4, 1400, 11),
    ("partial_sat", 256, 8, 1000, 5), ("vote_ties", 256, 5, 1400, 6), ("partial_sat", 256, 4, 1000, 7),
    ("vote_ties", 48, 8, 1400, 8), ("partial_sat", 48, 5, 1000, 9), ("vote_ties", 48, 4, 1400, 10),
    ("partial_sat", 80, 8, 1000, 11), ("vote_ties", 80, 5, 1400, 5), ("partial_sat", 80, 4, 1000, 6),
    ("vote_ties", 272, 8, 1400, 7), ("partial_sat", 272, 5, 1001, 8), ("vote_ties", 272, 4, 1400, 9),
    ("partial_sat", 1040, 8, 1000, 10), ("vote_ties", 1040, 5, 1406, 11), ("partial_sat", 1040, 4, 1000, 5),
    ("partial_sat", 64, 8, 1000, 40),
]
# one pin where the rejecting cost is a SATURATED one: some pixel of this frame is accepted at u and rejected at u + 1, and every
# cost that rejects it there is 32767 (32767 (100 - u - 1) < minS 100 <= 32767 (100 - u)); 14 pixels of the map change
SAT_PIN = ("partial_sat", 64, 8, 1000, 40)


def pins(D, paths):
    return [p for p in PINS if p[1] == D and p[2] == paths]
