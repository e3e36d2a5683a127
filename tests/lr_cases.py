"""The cases of the left-right check's state tests: tests/test_lr_states_cpu.py (the model against the oracle, the census
floors, the wrong variants, all without a device), tests/test_rows_plan_cpu.py (the planned form of every case) and
tests/test_gpu_lr_states.py (every case through HIPMatcher against the oracle, bit for bit).

A case is a dict: sec (A .. E), name, scene, W, H, D, w, cap, minD, M (disp12MaxDiff), window (speckleWindowSize; 0: the check
runs without the speckle filter's fused row init), range (speckleRange), n (frames in the call), roi (ROI1 or None), and what
plan_lrcheck must plan for it: form and init.  textureThreshold and uniquenessRatio are 0 everywhere, so that every pixel the
search computes reaches the check.  GROUPS collects the cases by (form, init): the census floors and the separation of the
wrong variants hold per group -- no single scene holds every state.

What cannot be reached: the W + 2 < 16384 bound of two_ok_for_pk and the 64 KB LDS bound beside it (rtdm_bm_create refuses
frames wider than 4096, where the packed form's LDS is 24.6 KB), and the scalar_u16 form (row 24 of DESIGN.md's route table).
"""
import functools

import numpy as np

import hostile_pairs as hp
import lr_model as lm
import lr_scenes as ls

FORMS = ("scalar_u16", "scalar_i32", "vec_wave", "vec_half", "vec_half2", "packed")
CASES = []


def case(sec, name, scene, W, H, D, w, cap, form, init, M=1, minD=0, window=0, range_=32, n=1, roi=None, thin=False):
    assert form in FORMS and init == (window > 0)
    c = dict(sec=sec, name=name, scene=scene, W=W, H=H, D=D, w=w, cap=cap, minD=minD, M=M, window=window, range=range_, n=n,
             roi=roi, form=form, init=init, thin=thin)
    c["id"] = "%s-%s-%s%s" % (sec, name, form, "-init" if init else "")
    CASES.append(c)
    return c


def hpair(family, seed):
    return ("hp", family, seed)


# ---- A. every decision on every reachable form, with and without the fused speckle init -----------------------------------
#        (tag, W, H, D, w, cap, window, n, form)
A_SHAPES = [("pk", 300, 40, 64, 9, 31, 0, 1, "packed"),
            ("pk3rows", 300, 11, 64, 9, 31, 2, 1, "packed"),              # fewer than 4 rows: no block of two row pairs
            ("pkbatch", 1032, 98, 64, 9, 31, 2, 129, "packed"),           # W > 1024 and n nrows > 11520
            ("half2", 300, 40, 64, 9, 31, 2, 1, "vec_half2"),
            ("half", 300, 48, 64, 21, 63, 0, 1, "vec_half"),              # 2 cap w w = 55566: not packed, 16-bit costs
            ("half3rows", 300, 23, 64, 21, 63, 2, 1, "vec_half"),
            ("wave", 2064, 16, 16, 5, 31, 0, 1, "vec_wave"),              # 9 half-waves of chunks
            ("waveinit", 2064, 16, 16, 5, 31, 2, 1, "vec_wave"),
            ("i32", 260, 40, 64, 25, 63, 0, 1, "scalar_i32"),             # 2 cap w w = 78750: 32-bit costs
            ("i32init", 260, 40, 64, 25, 63, 2, 1, "scalar_i32")]
A_SCENES = [("steps-M0", hpair("steps", 4), 0, 0), ("steps-M1", hpair("steps", 8), 1, 0), ("steps-M2", hpair("steps", 8), 2, 0),
            ("ties", hpair("ties", 3), 1, 0), ("worst_noise", hpair("worst_noise", 8), 1, 0), ("steps-minD-7", hpair("steps", 8), 1, -7)]
for tag, W, H, D, w, cap, window, n, form in A_SHAPES:
    for sname, scene, M, minD in A_SCENES:
        case("A", "%s-%s" % (tag, sname), scene, W, H, D, w, cap, form, window > 0, M=M, minD=minD, window=window, n=n)

# ---- B / C1. the cost's top bits, and either side of 2 cap w w < 32768 ------------------------------------------------------
SAW = ("saw", 0.01, 8)
SAW_MIXED = ("saw", 0.1, 8)            # a tenth of the pixels noise: the winners' costs lie on both sides of 32768 at w 21, cap 63
for w, cap, form in ((17, 56, "packed"), (17, 57, "vec_half"), (21, 37, "packed"), (21, 38, "vec_half"), (21, 63, "vec_half")):
    case("BC1", "saw-w%d-cap%d" % (w, cap), SAW, 300, 48, 64, w, cap, form, False)
    case("BC1", "saw-w%d-cap%d-3rows" % (w, cap), SAW, 300, w + 2, 64, w, cap, form, True, window=2)
case("B", "saw-half2", SAW, 300, 48, 64, 21, 63, "vec_half2", True, window=2)
case("B", "saw-wave", SAW, 2064, 32, 16, 21, 63, "vec_wave", False)
case("B", "saw-waveinit", SAW, 2064, 32, 16, 21, 63, "vec_wave", True, window=2)
case("B", "saw-i32", SAW, 260, 40, 64, 25, 63, "scalar_i32", False)
case("B", "saw-i32init", SAW, 260, 40, 64, 25, 63, "scalar_i32", True, window=2)
# costs on both sides of 32768 that compete for one slot: what a form that compared them as int16 would get wrong
case("B", "sawmixed-half", SAW_MIXED, 300, 48, 64, 21, 63, "vec_half", False)
case("B", "sawmixed-half3rows", SAW_MIXED, 300, 23, 64, 21, 63, "vec_half", True, window=2)
case("B", "sawmixed-half2", SAW_MIXED, 300, 48, 64, 21, 63, "vec_half2", True, window=2)
case("B", "sawmixed-wave", SAW_MIXED, 2064, 32, 16, 21, 63, "vec_wave", False)
case("B", "sawmixed-waveinit", SAW_MIXED, 2064, 32, 16, 21, 63, "vec_wave", True, window=2)
case("B", "sawmixed-i32", ("saw", 0.5, 8), 260, 40, 64, 25, 58, "scalar_i32", False)       # 2 cap w w = 72500
case("B", "sawmixed-i32init", ("saw", 0.5, 8), 260, 40, 64, 25, 58, "scalar_i32", True, window=2)

# ---- C2. disp12MaxDiff 512 | 513 on the cliffs, 511 and 520 so that the threshold itself is live -------------------------------
for M, form in ((511, "packed"), (512, "packed"), (513, "vec_half"), (519, "vec_half"), (520, "vec_half")):
    case("C2", "cliffs-M%d" % M, ("cliffs", 8), 1400, 16, 640, 9, 31, form, False, M=M)

# ---- C3 / C4. minDisparity -1024 | -1025 and minDisparity + numDisparities 1024 | 1025 ------------------------------------------
for fam in ("steps", "plateau_noise"):
    case("C3", "%s-minD-1024" % fam, hpair(fam, 8), 1200, 20, 64, 9, 31, "packed", False, minD=-1024)
    case("C3", "%s-minD-1025" % fam, hpair(fam, 8), 1208, 20, 64, 9, 31, "vec_half", False, minD=-1025)
    case("C4", "%s-minD960" % fam, hpair(fam, 8), 2040, 20, 64, 9, 31, "packed", False, minD=960, thin=True)
    case("C4", "%s-minD961" % fam, hpair(fam, 8), 2040, 20, 64, 9, 31, "vec_half", False, minD=961, thin=True)
case("C3", "steps-minD-1024-3rows", hpair("steps", 8), 1200, 11, 64, 9, 31, "packed", True, minD=-1024, window=2)
case("C3", "steps-minD-1025-3rows", hpair("steps", 8), 1208, 11, 64, 9, 31, "vec_half", True, minD=-1025, window=2)

# ---- C5. speckleRange 4096 | 4097 on the packed form with the init (3 rows) ----------------------------------------------------
C5_WINDOW = 60          # a strip of 16 columns x 3 rows is a speckle unless it hangs on to an anchor (48 columns x 3 rows)
for rng_, form in ((4095, "packed"), (4096, "packed"), (4097, "vec_half")):
    case("C5", "range%d" % rng_, ("rsteps", 9), 1032, 11, 320, 9, 31, form, True, window=C5_WINDOW, range_=rng_)

# ---- D. the ends of int16 ---------------------------------------------------------------------------------------------------
for fam in ("steps", "plateau_noise"):
    for window in (0, 2):
        case("D", "%s-minD-2047-win%d" % (fam, window), hpair(fam, 8), 2200, 14, 16, 5, 31, "vec_wave", window > 0, minD=-2047, window=window)
        case("D", "%s-minD2031-win%d" % (fam, window), hpair(fam, 8), 4096, 24, 16, 5, 31, "vec_wave", window > 0, minD=2031, window=window,
             thin=True)

# ---- a range that straddles -1024 (x16: -16384) on every form the plan lets see one: four frames, disp12MaxDiff 2 -----------
for tag, W, H, D, w, cap, window, minD, form in (("half", 1208, 48, 64, 21, 63, 0, -1056, "vec_half"),
                                                 ("half3rows", 1208, 23, 64, 21, 63, 2, -1056, "vec_half"),
                                                 ("half2", 1208, 20, 64, 9, 31, 2, -1056, "vec_half2"),
                                                 ("wave", 2200, 14, 16, 5, 31, 0, -1032, "vec_wave"),
                                                 ("waveinit", 2200, 14, 16, 5, 31, 2, -1032, "vec_wave"),
                                                 ("i32", 1208, 40, 64, 25, 63, 0, -1056, "scalar_i32"),
                                                 ("i32init", 1208, 40, 64, 25, 63, 2, -1056, "scalar_i32")):
    case("D", "straddle-%s" % tag, ("straddle", 8), W, H, D, w, cap, form, window > 0, M=2, minD=minD, window=window, n=4)

# ---- the one column per row that holds a disparity and may not vote, on every form: four frames ------------------------------
for tag, W, H, D, w, cap, window, n, form in A_SHAPES:
    if tag != "pkbatch":
        case("A", "%s-nonvoter" % tag, ("nv", 8), W, H, D, w, cap, form, window > 0, window=window, n=4)
        # ... and look-ups of the slot that holds its vote and no other
        case("A", "%s-nonvoter-only" % tag, ("nvramp", 8), W, H, D, w, cap, form, window > 0, window=window, n=4)

# ---- E. geometry --------------------------------------------------------------------------------------------------------------
for W in (233, 238, 239, 240):
    case("E", "W%d" % W, hpair("steps", 8), W, 40, 64, 9, 31, "packed", False)
    case("E", "W%d-init" % W, hpair("steps", 8), W, 40, 64, 9, 31, "vec_half2", True, window=2)
# ROI1 (x, y, w, h): the valid rectangle is columns [83, 221) -- it starts and ends inside a chunk of 8 -- and rows [7, 32):
# an odd first row, an odd row count
E_ROI = (79, 3, 146, 33)
case("E", "roi", hpair("steps", 8), 300, 40, 64, 9, 31, "packed", False, roi=E_ROI)
case("E", "roi-init", hpair("steps", 8), 300, 40, 64, 9, 31, "vec_half2", True, window=2, roi=E_ROI)
case("E", "batch3", hpair("steps", 8), 300, 40, 64, 9, 31, "packed", False, n=3)
case("E", "batch3-init", hpair("steps", 8), 300, 40, 64, 9, 31, "vec_half2", True, window=2, n=3)

assert len({c["id"] for c in CASES}) == len(CASES)
GROUPS = {}
for c in CASES:
    GROUPS.setdefault((c["form"], c["init"]), []).append(c)

# the top bit of the cost a form can be handed (section B): the packed form never sees bit 15 (two_ok_for_pk), no 16-bit form bit 16
COST_STATE = {"packed": "cost_ge_2_14", "vec_half": "cost_ge_2_15", "vec_half2": "cost_ge_2_15", "vec_wave": "cost_ge_2_15",
              "scalar_i32": "cost_ge_2_16"}
# variants no input of the form can show, because plan_lrcheck never hands the packed form such an input: costs at or above 32768
# (2 cap w w < 32768) and disparities outside +-16384 (minD >= -1024, minD + D <= 1024)
UNREACHABLE = {("packed", "cost_int16"), ("packed", "disp_wrap15")}
FLOOR, ALIVE, ALIVE_THIN = 5, 100, 50


# ---- frames ---------------------------------------------------------------------------------------------------------------------
def n_sources(c):
    """distinct frames of the call: a batch above four frames repeats four"""
    return min(c["n"], 4)


def source_of(c):
    """frame -> source frame; the last frame of a long batch is the last source"""
    idx = np.arange(c["n"]) % n_sources(c)
    idx[-1] = n_sources(c) - 1
    return idx


def compared(c):
    """the frames that are compared: all of up to four, the first and the last of a longer batch"""
    return tuple(range(c["n"])) if c["n"] <= 4 else (0, c["n"] - 1)


@functools.lru_cache(maxsize=None)
def _sources(scene, k, W, H, D, minD, w):
    kind, seed = scene[0], scene[-1]
    if kind == "hp":
        L, R = hp.make_n(scene[1], seed, k, W, H, D, minD, w)
    else:
        make = {"saw": lambda s: ls.sawtooth(s, W, H, scene[1]), "cliffs": lambda s: ls.cliffs(s, W, H),
                "rsteps": lambda s: ls.range_steps(s, W, H), "straddle": lambda s: ls.straddle(s, W, H),
                "nv": lambda s: ls.nonvoter(s, W, H, D, w, 5 if D > 16 else 2), "nvramp": lambda s: ls.nonvoter_ramp(s, W, H, D, w)}[kind]
        pairs = [make(seed + i) for i in range(k)]
        L, R = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    L.setflags(write=False); R.setflags(write=False)
    return L, R


def sources(c):
    """-> (L, R) uint8 [n_sources, H, W], read-only and shared"""
    return _sources(c["scene"], n_sources(c), c["W"], c["H"], c["D"], c["minD"], c["w"])


# ---- the oracle's side ------------------------------------------------------------------------------------------------------------
def oracle_kw(c, **over):
    kw = dict(numDisparities=c["D"], blockSize=c["w"], minDisparity=c["minD"], preFilterCap=c["cap"], textureThreshold=0,
              uniquenessRatio=0, disp12MaxDiff=c["M"], speckleWindowSize=c["window"], speckleRange=c["range"], roi1=c["roi"])
    kw.update(over)
    return kw


def want_map(oracle, c, L, R, **over):
    return oracle.bm_compute(L, R, nthreads=4, **oracle_kw(c, **over))


def raw_planes(oracle, c, L, R):
    """-> (rect, disp, cost): the valid rectangle (x, y, w, h) and what the search leaves on its rows, before the check"""
    kw = oracle_kw(c)
    rect = oracle.valid_rect(c["W"], c["H"], **kw)
    assert rect is not None, c["id"]
    disp, cost = oracle.bm_search(oracle.prefilter_xsobel(L, c["cap"]), oracle.prefilter_xsobel(R, c["cap"]), rect[1], rect[1] + rect[3], **kw)
    return rect, disp, cost


def finish(oracle, c, rect, checked):
    """what follows the check: the columns outside the valid rectangle, then the speckle filter"""
    inv = (c["minD"] - 1) * 16
    out = np.array(checked, np.int16)
    out[:, :rect[0]] = inv; out[:, rect[0] + rect[2]:] = inv
    if c["window"] > 0 and c["range"] >= 0:
        out = oracle.filter_speckles(out, inv, c["window"], c["range"])
    return out


def model_map(oracle, c, rect, disp, cost, variant=None):
    return finish(oracle, c, rect, lm.validate(disp, cost, c["W"], c["minD"], c["D"], c["M"], variant))
