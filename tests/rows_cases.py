"""The route table of the two row stages behind the StereoBM search (plan_lrcheck / plan_speckle in
rt-depth-map_amd/csrc/k_rows.hip; DESIGN.md, "K3 / K4: routes"), shared by tests/test_rows_plan_cpu.py, which pins every row
field by field, and tests/test_gpu_rows_routes.py, which runs a row of every kernel form against the oracle.

All rows: full frame, no ROI, minDisparity 0, speckleRange 32; unless a row says otherwise disp12MaxDiff 1,
speckleWindowSize 100, rows aligned, no environment hook.  nrows = H - (w - 1).

lr: (form, block threads, grid.y, dynamic LDS bytes, heads left for the filter, block_rows), None: the check is off.
spk: (k_spk_init runs, (where k_spk_merge_rec runs, its workgroups), merge form, grid.x, first, npairs, ystep), None: the
filter is off.  Count / apply run DENSE exactly where the heads are CHUNK, on a grid of (n H + 15) / 16."""


def row(no, W, H, D, w, cap, n, lr, spk, env=None, maxdiff=1, window=100, aligned=1):
    return dict(no=no, W=W, H=H, D=D, w=w, cap=cap, n=n, lr=lr, spk=spk, env=env or {}, maxdiff=maxdiff, window=window, aligned=aligned)


NO_REC = (None, 0)
_R1_LR = ("vec_half2", 128, 18, 4896, "CHUNK", 4)
_R3_LR = ("packed", 128, 36, 3680, "CHUNK", 1)
_R3_SPK = (False, NO_REC, "strip<1,chunk>", 11, 4, 71, 1)
_PAIRS1 = {"RTDM_LR_PAIRS": "1"}

BM_ROWS = [
    row("1", 300, 80, 64, 9, 31, 1, _R1_LR, (False, ("fused", 9), "strip<1,chunk,REC>", 12, 7, 17, 4)),
    row("2", 300, 80, 64, 9, 31, 1, _R1_LR, (False, ("own", 9), "strip<1,chunk>", 3, 7, 17, 4), env={"RTDM_MERGE_REC_FUSED": "0"}),
    row("3", 300, 80, 64, 9, 31, 1, _R3_LR, _R3_SPK, env=_PAIRS1),
    row("4", 300, 80, 64, 9, 31, 200, _R3_LR, (False, NO_REC, "strip<2,chunk>", 6, 4, 71, 1), env=_PAIRS1),
    row("5", 300, 80, 64, 9, 31, 400, _R3_LR, (False, NO_REC, "strip<4,chunk>", 3, 4, 71, 1), env=_PAIRS1),
    row("6", 300, 80, 64, 9, 31, 1, ("vec_half", 128, 36, 3680, "CHUNK", 1), _R3_SPK, env={"RTDM_LR_PAIRS": "1", "RTDM_LR_PACKED": "0"}),
    row("7", 300, 80, 64, 9, 31, 1, ("packed", 128, 36, 3680, "NONE", 1), None, window=0),
    row("8", 300, 80, 64, 9, 31, 1, None, (True, NO_REC, "strip<4,pixel>", 3, 0, 79, 1), maxdiff=-1),
    row("9", 300, 83, 64, 9, 31, 1, ("vec_half2", 128, 19, 4896, "CHUNK", 4), (False, ("fused", 9), "strip<1,chunk,REC>", 12, 7, 18, 4)),
    # nrows 4: one block, no pair left across blocks -- the rec pass runs on its own although fusing is on, and no strip
    row("10", 96, 12, 16, 9, 31, 1, ("vec_half2", 64, 1, 1568, "CHUNK", 4), (False, ("own", 1), "none", 0, 7, 0, 1)),
    row("11", 96, 11, 16, 9, 31, 1, ("packed", 64, 2, 1184, "CHUNK", 1), (False, NO_REC, "strip<1,chunk>", 1, 4, 2, 1)),      # nrows 3 < 4
    row("12", 233, 156, 64, 9, 31, 1, ("vec_half2", 64, 37, 3872, "CHUNK", 4), (False, ("fused", 14), "strip<1,chunk,REC>", 19, 7, 36, 4)),   # ragged: Ws 240
    row("13", 1032, 98, 64, 9, 31, 128, ("vec_half2", 320, 23, 16544, "CHUNK", 4), (False, ("fused", 34), "strip<1,chunk,REC>", 46, 7, 22, 4)),   # n nrows = 11520
    row("14", 1032, 98, 64, 9, 31, 129, ("packed", 320, 45, 12416, "CHUNK", 1), (False, NO_REC, "strip<4,chunk>", 12, 4, 89, 1)),
    row("15", 1024, 98, 64, 9, 31, 129, ("vec_half2", 256, 23, 16416, "CHUNK", 4), (False, ("fused", 34), "strip<1,chunk,REC>", 45, 7, 22, 4)),   # W <= 1024
    # 2 cap w^2 = 36414 >= 32768: not packed
    row("16", 1032, 106, 64, 17, 63, 129, ("vec_half", 320, 45, 12416, "CHUNK", 1), (False, NO_REC, "strip<4,chunk>", 12, 8, 89, 1)),
    row("17", 2048, 40, 16, 5, 31, 1, ("vec_half2", 512, 9, 32800, "CHUNK", 4), (False, ("fused", 27), "strip<1,chunk,REC>", 35, 5, 8, 4)),   # 8 half-waves
    row("18", 2064, 40, 16, 5, 31, 1, ("vec_wave", 320, 36, 12400, "CHUNK", 1), (False, NO_REC, "strip<1,chunk>", 36, 2, 35, 1)),   # 9 half-waves
    row("19", 260, 80, 64, 23, 63, 1, ("scalar_i32", 256, 58, 3120, "PIXEL", 1), (False, NO_REC, "strip<4,pixel>", 2, 11, 57, 1)),   # costs past 16 bits
    row("20", 1280, 720, 64, 9, 31, 1, ("vec_half2", 320, 178, 20512, "CHUNK", 4), (False, ("fused", 334), "strip<1,chunk,REC>", 445, 7, 177, 4)),
    row("21a", 1280, 720, 64, 9, 31, 16, ("vec_half2", 320, 178, 20512, "CHUNK", 4), (False, ("fused", 334), "strip<1,chunk,REC>", 445, 7, 177, 4)),
    row("21b", 1280, 720, 64, 9, 31, 17, ("packed", 320, 356, 15392, "CHUNK", 1), (False, NO_REC, "strip<4,chunk>", 112, 4, 711, 1)),
    # the shape of the two batches of tests/test_gpu_speckle_extruded.py (31 row pairs of 80 chunks): strips of four pairs are
    # 3 workgroups per frame, 3 n >= 1024 from n = 342; strips of two are 5, 5 n >= 1024 from n = 205
    row("x352", 640, 40, 64, 9, 31, 352, ("packed", 192, 16, 7712, "CHUNK", 1), (False, NO_REC, "strip<4,chunk>", 3, 4, 31, 1), env=_PAIRS1),
    row("x208", 640, 40, 64, 9, 31, 208, ("packed", 192, 16, 7712, "CHUNK", 1), (False, NO_REC, "strip<2,chunk>", 5, 4, 31, 1), env=_PAIRS1),
    # rows that are not aligned (no ABI entry hands such a plane over): the scalar kernels, W (4 + 2 + 2) bytes of LDS
    row("24", 300, 80, 64, 9, 31, 1, ("scalar_u16", 256, 72, 2400, "PIXEL", 1), (False, NO_REC, "rows", 11, 4, 71, 1), aligned=0),
]
# the StereoSGBM hand-off (sgm_finish: PIXEL heads, nothing merged, every row, workspace rows of W elements): (no, W, H, n, spk)
SGM_ROWS = [("22", 640, 480, 1, (False, NO_REC, "strip<4,pixel>", 38, 0, 479, 1)),
            ("23", 644, 480, 1, (False, NO_REC, "rows", 152, 0, 479, 1))]                  # Ws % 8 != 0

GPU_ROWS = ("1", "7", "8", "9", "10", "11", "12", "14", "16", "18", "19")
# rows 10 and 11 are three and four rows of 96 columns: a window of 100 would remove everything
GPU_WINDOW = {"10": 30, "11": 30}
SEED_BASE = 700


def gpu_rows():
    out = []
    for r in BM_ROWS:
        if r["no"] in GPU_ROWS:
            assert not r["env"]
            out.append(dict(r, window=GPU_WINDOW.get(r["no"], r["window"])))
    assert len(out) == len(GPU_ROWS)
    return out


def frames(r):
    """the frames of a batch that are compared: all of a single frame, the first and the last of a batch"""
    return (0,) if r["n"] == 1 else (0, r["n"] - 1)


def stream(synth, r):
    return synth.make_stream(SEED_BASE + r["D"] + r["w"], r["n"], r["W"], r["H"], r["D"])


def oracle_kw(r, **over):
    kw = dict(numDisparities=r["D"], blockSize=r["w"], preFilterCap=r["cap"], disp12MaxDiff=r["maxdiff"], speckleWindowSize=r["window"],
              speckleRange=32)
    kw.update(over)
    return kw


def liveness(oracle, r, L, R):
    """-> (the oracle's map, pixels the left-right check removes, pixels the speckle filter removes, pixels that survive),
    from the oracle alone: the difference between its runs with a stage on and off.  A stage the row does not run counts None."""
    inv = -16
    want = oracle.bm_compute(L, R, nthreads=8, **oracle_kw(r))
    lr = spk = None
    checked = want if r["window"] <= 0 else oracle.bm_compute(L, R, nthreads=8, **oracle_kw(r, speckleWindowSize=0))
    if r["maxdiff"] >= 0:
        raw = oracle.bm_compute(L, R, nthreads=8, **oracle_kw(r, disp12MaxDiff=-1, speckleWindowSize=0))
        lr = int(((raw != inv) & (checked == inv)).sum())
    if r["window"] > 0:
        spk = int(((checked != inv) & (want == inv)).sum())
    return want, lr, spk, int((want != inv).sum())


def assert_live(r, frame, lr, spk, alive):
    what = "row %s frame %d: the left-right check removes %s, the speckle filter %s, %d survive" % (r["no"], frame, lr, spk, alive)
    assert lr is None or lr >= 5, what
    assert spk is None or spk >= 5, what
    assert alive >= 100, what
    return what
