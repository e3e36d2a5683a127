"""The cases of tests/lr_cases.py without a device: that the model of tests/lr_model.py IS the oracle's left-right check on every
one of them, that every decision the check can take is live in every group of cases that share a kernel form and a speckle-init
setting, and that each group tells every deliberately wrong variant of the model from the oracle on the final map -- the
evidence that tests/test_gpu_lr_states.py, which runs the same cases on the device, would notice such a kernel.

Floors (rows_cases.assert_live's): 5 pixels per state and group, 100 surviving pixels in every compared frame (50 on the two
thin shapes, whose valid rectangle is 15 and 49 columns wide).  With the speckle filter on, only pixels whose final value is the
checked one are counted."""
import functools

import numpy as np
import pytest

import lr_cases as lc
import lr_model as lm
import lr_scenes as ls

REQUIRED = lm.PIXEL_STATES + ("nonvoter",)
BY_ID = {c["id"]: c for c in lc.CASES}
GROUP_IDS = ["%s%s" % (f, "-init" if i else "") for f, i in lc.GROUPS]


@functools.lru_cache(maxsize=None)
def _report(oracle, cid):
    """per compared frame: (model == oracle's check, model pipeline == oracle's map, census, {variant: differing pixels}, survivors)"""
    c = BY_ID[cid]
    L, R = lc.sources(c)
    src = lc.source_of(c)
    inv = (c["minD"] - 1) * 16
    out = []
    for f in lc.compared(c):
        s = src[f]
        rect, disp, cost = lc.raw_planes(oracle, c, L[s], R[s])
        checked = lm.validate(disp, cost, c["W"], c["minD"], c["D"], c["M"])
        same_check = np.array_equal(checked, oracle.validate_disparity(disp, cost, c["minD"], c["D"], c["M"]))
        want = lc.want_map(oracle, c, L[s], R[s])
        same_map = np.array_equal(lc.finish(oracle, c, rect, checked), want)
        keep = want == lc.finish(oracle, dict(c, window=0), rect, checked)       # the filter left the checked value
        census = lm.census(disp, cost, c["W"], c["minD"], c["D"], c["M"], rect, keep)
        sep = {v: int((lc.model_map(oracle, c, rect, disp, cost, v) != want).sum()) for v in lm.VARIANTS}
        out.append((same_check, same_map, census, sep, int((want != inv).sum())))
    return out


@pytest.mark.parametrize("cid", list(BY_ID))
def test_model_is_the_oracle_and_frames_survive(oracle, cid):
    c = BY_ID[cid]
    for f, (same_check, same_map, census, sep, alive) in zip(lc.compared(c), _report(oracle, cid)):
        what = "%s frame %d: %d survive, census %s" % (cid, f, alive, census)
        print(what)
        assert same_check, what                       # validate() == orc_validate_disparity, bit for bit
        assert same_map, what                         # ... and search, validate(), rectangle, speckle filter == orc_bm_compute
        assert alive >= (lc.ALIVE_THIN if c["thin"] else lc.ALIVE), what


@pytest.mark.parametrize("group", list(lc.GROUPS), ids=GROUP_IDS)
def test_every_state_is_live_in_every_group(oracle, group):
    form, init = group
    total = {}
    for c in lc.GROUPS[group]:
        for _, _, census, _, _ in _report(oracle, c["id"]):
            for k, v in census.items():
                total[k] = max(total.get(k, 0), v) if k == "max_cost" else total.get(k, 0) + v
    print(group, total)
    for state in REQUIRED + (lc.COST_STATE[form],):
        assert total[state] >= lc.FLOOR, (group, state, total)
    # what the plan never hands the form (lr_cases.COST_STATE)
    assert form != "packed" or total["cost_ge_2_15"] == 0
    assert form == "scalar_i32" or total["cost_ge_2_16"] == 0


@pytest.mark.parametrize("group", list(lc.GROUPS), ids=GROUP_IDS)
def test_every_wrong_variant_differs_from_the_oracle_in_every_group(oracle, group):
    form, init = group
    total = dict.fromkeys(lm.VARIANTS, 0)
    for c in lc.GROUPS[group]:
        for _, _, _, sep, _ in _report(oracle, c["id"]):
            for v, k in sep.items():
                total[v] += k
    print(group, total)
    for v in lm.VARIANTS:
        if (form, v) in lc.UNREACHABLE:
            assert total[v] == 0, (group, v, total)       # no input the plan lets through can show it
        else:
            assert total[v] >= lc.FLOOR, (group, v, total)


def test_sections_reach_what_they_are_for(oracle):
    sec = lambda s: [c for c in lc.CASES if c["sec"] == s]
    # B: the cost's top bits on every form
    for c in lc.CASES:
        if c["scene"][0] == "saw" and c["scene"][1] == 0.01:
            census = _report(oracle, c["id"])[0][2]
            assert census[lc.COST_STATE[c["form"]]] >= lc.FLOOR or c["cap"] in (57, 38), (c["id"], census)
            assert census["both_disagree"] >= lc.FLOOR and census["second_agrees"] >= lc.FLOOR, (c["id"], census)
    # C2: the cliffs -- the threshold itself is live at 512 and at 520, and the check removes less and less
    kills = {c["M"]: _report(oracle, c["id"])[0][2] for c in sec("C2")}
    assert kills[512]["diff_eq_M"] >= 100 and kills[520]["diff_eq_M"] >= 100, kills
    assert kills[511]["both_disagree"] > kills[512]["both_disagree"] + 100 > kills[513]["both_disagree"] + 100, kills
    assert kills[519]["both_disagree"] > kills[520]["both_disagree"] + 100, kills
    assert kills[512]["won_tie"] >= 1000
    # C5: the oracle's maps at speckleRange 4095, 4096 and 4097 differ pairwise
    c5 = {c["range"]: c for c in sec("C5")}
    L, R = lc.sources(c5[4096])
    maps = {r: lc.want_map(oracle, c, L[0], R[0]) for r, c in c5.items()}
    for a, b in ((4095, 4096), (4096, 4097), (4095, 4097)):
        assert int((maps[a] != maps[b]).sum()) >= lc.FLOOR, (a, b)
    d = ls.range_steps_disparities(1032, 6)
    assert {256, 257} <= set(np.abs(np.diff(d)).tolist())
    # D: the disparities sit at the ends of int16, the invalid value of the lower end is -32768
    for c in sec("D"):
        if c["minD"] in (-2047, 2031):
            L, R = lc.sources(c)
            want = lc.want_map(oracle, c, L[0], R[0])
            inv = (c["minD"] - 1) * 16
            valid = want[want != inv]
            assert (inv == -32768 and valid.min() >= -32760 and valid.max() < -32500) if c["minD"] < 0 else (valid.min() > 32480 and valid.max() <= 32751)
    # E: the ROI's rectangle starts and ends inside a chunk of 8, on an odd row, with an odd row count
    roi = next(c for c in sec("E") if c["roi"])
    x, y, w, h = oracle.valid_rect(roi["W"], roi["H"], **lc.oracle_kw(roi))
    assert x % 8 and (x + w) % 8 and y % 2 == 1 and h % 2 == 1
