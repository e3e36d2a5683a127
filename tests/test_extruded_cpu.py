"""The extruded inputs of the speckle tests, checked on the CPU oracle alone: what tests/test_gpu_speckle_extruded.py assumes
about them holds, and the reference filter itself is pinned on these layouts by two further implementations."""
import numpy as np
import pytest

import bruteforce
import extruded as E


@pytest.fixture(scope="module")
def jobs(oracle):
    # the generators assert the conditions (queue overflow, rescue depth, exact sizes, hv boundary) as they go
    return {j["name"]: j for j in list(E.single_frame_jobs(oracle)) + list(E.batch_jobs(oracle))}


def test_every_input_meets_its_conditions_on_the_oracles_map(jobs):
    assert len(jobs) == 2 + 5 + 14 + 4 + 4
    for name in ("overflow640", "overflow1280", "heads640", "heads644", "scalar_lr") + tuple("batch_s%d" % s for s in E.BATCH_SEEDS):
        m = jobs[name]["measured"]
        contacts = m["contacts"] if isinstance(m["contacts"], int) else min(m["contacts"].values())
        assert contacts >= 1280 and m["hv_boundary"] >= 1000, (name, m)
    for bands, r, w in E.MARK_CASES:
        n, depth = jobs["marks_r%d_w%d" % (r, w)]["measured"]["rescue"]
        assert n >= 2000 and depth >= 12, (r, w, n, depth)
    at, above = jobs["marks_r0_w3"]["measured"]["exact"]
    assert at >= 100 and above >= 100
    rows = sorted(j["vy1"] - j["vy0"] for n, j in jobs.items() if n.startswith("rows_") and n.endswith("_o0") or n == "rows_h10_o1")
    assert rows == [1, 2, 3, 4, 5, 6, 7, 8, 9, 16, 33], rows
    assert sorted(jobs["rows_h%d_o%d" % (E.ROI_HEIGHT, o)]["vy0"] for o in E.ROI_OFFSETS) == [4, 5, 6, 7]


def test_interior_rows_of_a_band_are_identical(jobs):
    for name, j in jobs.items():
        assert E.interior_rows_identical(j, j["kw"]["blockSize"] // 2), name


def test_contact_count_is_the_number_of_unions_a_row_pair_needs(jobs):
    # new_run_contacts against its definition, pixel by pixel, on two rows of a map with runs of every length
    j = jobs["marks_r1_w8"]
    d, FIL, md = j["d"].astype(int), j["FIL"], j["maxDiff"]
    cand = E.new_run_contacts(d, FIL, md)
    run = lambda y: np.cumsum([d[y, x] != FIL and not (x > 0 and d[y, x - 1] != FIL and abs(d[y, x] - d[y, x - 1]) <= md)
                               for x in range(d.shape[1])])
    for y in (30, 64):
        ra, rb = run(y - 1), run(y)
        want, prev = [], None
        for x in range(d.shape[1]):
            c = d[y, x] != FIL and d[y - 1, x] != FIL and abs(d[y, x] - d[y - 1, x]) <= md
            want.append(bool(c and prev != (ra[x], rb[x])))
            prev = (ra[x], rb[x]) if c else None
        assert cand[y].tolist() == want
    assert not cand[0].any()


def test_workgroup_count_takes_256_chunks_row_major():
    cand = np.zeros((6, 20), bool)          # 3 chunks per row
    cand[1, :] = True; cand[2, 16:] = True; cand[5, 3] = True
    assert E.max_contacts_per_workgroup(cand, [1, 2]) == 24
    assert E.max_contacts_per_workgroup(cand, [5]) == 1
    assert E.max_contacts_per_workgroup(cand, []) == 0
    big = np.ones((200, 16), bool)          # 2 chunks per row: a workgroup takes 128 rows
    assert E.max_contacts_per_workgroup(big, range(1, 200)) == 128 * 16


def test_rescue_depth_on_a_hand_made_map():
    FIL = -16
    d = np.full((8, 12), FIL, np.int16)
    d[0, 0:6] = 100                          # a run of 6 ...
    d[1:6, 2] = 100                          # ... with a column of 5 hanging from it
    d[7, 8:10] = 50                          # and a run of 2 on its own
    assert E.rescue_depth(d, FIL, 0, 4) == (5, 5)
    assert E.rescue_depth(d, FIL, 0, 6) == (0, 0)
    lab, sizes = E.components(d, FIL, 0)
    assert sorted(sizes[sizes > 0].tolist()) == [2, 11] and (lab[d == FIL] == -1).all()
    assert E.band_height(d, FIL, 0, 8) == 6


def test_sgm_inputs_carry_marks_and_overflow_the_strip_queue(oracle):
    # StereoSGBM filters with 16 * speckleRange.  (0, 3): marks travel as under StereoBM; a thread of the per-pixel-head strip
    # kernel walks four row pairs, so at a width that is a multiple of 8 a workgroup meets well over the queue's 1024
    # contacts (one pair per thread would stay below: 727 .. 771).  (1, 20): one component covers the frame.
    for W in (640, 644):
        L, R = E.sgm_frames(W)
        for paths in (8, 5):
            d = oracle.sgm_compute(L, R, speckleWindowSize=0, speckleRange=0, paths=paths, **E.SGM)
            n, depth = E.rescue_depth(d, -16, 0, 3)
            assert n >= E.RESCUED_MIN and depth >= E.DEPTH_MIN, (W, paths, n, depth)
            cand = E.new_run_contacts(d, -16, 0)
            if W % 8 == 0:
                assert E.max_contacts_per_workgroup(cand, range(1, d.shape[0]), 4) >= E.OVERFLOW_MIN
            assert E.max_contacts_per_workgroup(cand, range(1, d.shape[0])) < E.QCAP
    L, R = E.sgm_frames(640, one_band=True)
    d = oracle.sgm_compute(L, R, speckleWindowSize=0, speckleRange=0, paths=8, **E.SGM)
    hv = E.band_height(d, -16, 0, d.shape[0])
    assert hv == 40 and E.require_hv_boundary(oracle, d, -16, 0, hv) >= 1000


CPU_MAPS = ("overflow640", "marks_r0_w3", "marks_r1_w8")        # 640 x 40 and 640 x 88: bruteforce.speckle is Python


@pytest.mark.parametrize("name", CPU_MAPS)
@pytest.mark.parametrize("rng_", [0, 1, 2])
def test_three_filters_agree_on_extruded_maps(oracle, jobs, name, rng_):
    j = jobs[name]
    d = E.unfiltered(oracle, j["L"], j["R"], **dict(j["kw"], speckleRange=rng_))
    y0, y1 = list(E.band_spans(j["bands"]))[len(j["bands"]) // 2]
    hv = E.band_height(d, j["FIL"], y0, y1)
    assert hv == (40 if len(j["bands"]) > 1 else 32)
    changed = 0
    for win in (hv - 1, hv, 2 * hv - 1, 2 * hv, 3, 20):
        a = oracle.filter_speckles(d, j["FIL"], win, rng_)
        assert np.array_equal(a, bruteforce.speckle(d, j["FIL"], win, rng_)), (name, rng_, win, "label propagation")
        assert np.array_equal(a, E.filter_by_components(d, j["FIL"], rng_, win)), (name, rng_, win, "csgraph")
        # and through the whole matcher: speckleWindowSize = win is the filter applied to the unfiltered map
        assert np.array_equal(a, oracle.bm_compute(j["L"], j["R"], nthreads=8, **dict(j["kw"], speckleRange=rng_, speckleWindowSize=win)))
        changed += int((a != d).sum())
    assert changed > 0, "no window removed a pixel"
