"""What plan_sgm_cost (rt-depth-map_amd/csrc/rtdm_sgm_cost_plan.h) plans for the cost stage of a StereoSGBM call, through the
stand-alone program tests/sgm_cost_plan_host.cpp: built with the host compiler from the one header (no HIP, nothing to link), a
second time with -fsanitize=address,undefined.  PLAIN holds the rows of DESIGN.md ("SGM: cost routes"); the model below restates
the branch nest that the plan replaced (the old launch_sgm_cost with its launch_box, launch_sgm_warm3, sgm_cost16_needed and the
C ABI layer's sgm_cost_limit) as the kernel launches it issued, and the program is swept against it.  The device cases of
sgm_cost_routes.py are held to their rows here, and their expected frames to being live, different and not refused."""
import itertools
import os
import subprocess

import pytest

import sgm_cost_routes as routes
from conftest import PKG, ROOT

CENSUS_WINDOWS = [(cw, ch) for cw in (3, 5, 7, 9) for ch in (3, 5, 7)]


def build(tmp, name, extra):
    out = str(tmp / name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror"] + extra +
                          ["-I", os.path.join(ROOT, PKG, "csrc"), os.path.join(ROOT, "tests", "sgm_cost_plan_host.cpp"), "-o", out])
    return out


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build(tmp_path_factory.mktemp("sgm_cost_plan"), "sgm_cost_plan_host", [])


@pytest.fixture(scope="module")
def exe_san(tmp_path_factory):
    return build(tmp_path_factory.mktemp("sgm_cost_plan_san"), "sgm_cost_plan_host_san",
                 ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                  "-static-libasan", "-static-libubsan"])     # (the runtimes inside the executable: nothing to preload, no link order)


def cfg(D=16, H=12, bs=5, P2=2400, cn=1, ftz=15, census=None, paths=5, f16=0):
    """-> the program's eleven numbers"""
    cw, ch = census or (9, 7)
    return (D, H, bs, P2, cn, ftz, int(census is not None), cw, ch, paths, f16)


def run(exe, cfgs):
    """-> one dict per configuration: variant and the printed fields (numbers as ints); the configurations travel on standard input"""
    text = "".join(" ".join(str(v) for v in c) + "\n" for c in cfgs)
    p = subprocess.run([exe, "-"], input=text, capture_output=True, text=True)
    assert p.returncode == 0 and not p.stderr, p.stdout[-2000:] + p.stderr[-4000:]
    out = []
    for line in p.stdout.splitlines():
        variant, rest = line.split(" ", 1)
        f = dict(kv.split("=") for kv in rest.split(" "))
        out.append(dict({k: (int(v) if v.lstrip("-").isdigit() else v) for k, v in f.items()}, variant=variant))
    assert len(out) == len(cfgs)
    return out


# ---- the table.  (number, configuration, form, sum, R, records, volume, limit); check = limit > 0; ftz / cw / ch as given.
# Rows 21 - 40: the configuration of row - 20 under paths = 3 -- the same plan with warm = 1, wrows = min(R, H) and "_w3".
BIG = 30000
PLAIN = [
    (1, cfg(D=64, bs=7), "BT8", "FUSED", 3, 8, "NONE", 0),
    (2, cfg(D=48, bs=3), "BT8", "BOX", 1, 8, "PIX", 0),
    (3, cfg(D=16, bs=7, P2=BIG), "BT8", "BOX", 3, 8, "PIX", 2767),
    (4, cfg(D=16, bs=19), "BT8", "BOX_ANY", 9, 8, "PIX", 30367),
    (5, cfg(D=128, bs=5, f16=1), "BT16_GRAY", "FUSED", 2, 8, "NONE", 0),
    (6, cfg(D=32, bs=5, ftz=97, P2=BIG), "BT16_GRAY", "FUSED", 2, 8, "NONE", 2767),
    (7, cfg(D=16, bs=13, f16=1), "BT16_GRAY", "BOX", 6, 8, "S", 0),
    (8, cfg(D=16, bs=13, ftz=97), "BT16_GRAY", "BOX", 6, 8, "S", 30367),
    (9, cfg(D=16, bs=15, f16=1), "BT16_GRAY", "BOX_ANY", 7, 8, "S", 0),
    (10, cfg(D=16, bs=15, ftz=97), "BT16_GRAY", "BOX_ANY", 7, 8, "S", 30367),
    (11, cfg(D=256, bs=3, cn=3), "BT16_COLOUR", "FUSED", 1, 24, "NONE", 0),
    (12, cfg(D=16, bs=3, cn=3, P2=31000), "BT16_COLOUR", "FUSED", 1, 24, "NONE", 1767),
    (13, cfg(D=16, bs=9, cn=3), "BT16_COLOUR", "BOX", 4, 24, "S", 0),
    (14, cfg(D=272, bs=13, cn=3), "BT16_COLOUR", "BOX", 6, 24, "S", 30367),
    (15, cfg(D=16, bs=15, cn=3), "BT16_COLOUR", "BOX_ANY", 7, 24, "S", 30367),
    (16, cfg(D=16, bs=3, census=(9, 7), f16=1), "CENSUS", "FUSED", 1, 8, "NONE", 0),
    (17, cfg(D=16, bs=17, census=(9, 7)), "CENSUS", "BOX", 8, 8, "PIX", 0),
    (18, cfg(D=16, bs=17, census=(9, 7), P2=16000), "CENSUS", "BOX", 8, 8, "PIX", 16767),
    (19, cfg(D=16, bs=19, census=(9, 7)), "CENSUS", "BOX_ANY", 9, 8, "PIX", 0),
    (20, cfg(D=16, bs=19, census=(9, 7), P2=12000), "CENSUS", "BOX_ANY", 9, 8, "PIX", 20767),
]


def expected(row, warm, H=12):
    num, c, form, ssum, R, records, volume, limit = row
    census = form == "CENSUS"
    warm = int(warm and R > 0)
    return dict(variant=routes.ROWS[num] + ("_w3" if warm else ""), form=form, sum=ssum, R=R, records=records, volume=volume,
                check=int(limit > 0), limit=limit, warm=warm, wrows=min(R, H) if warm else 0, ftz=0 if census else c[5],
                cw=c[7] if census else 0, ch=c[8] if census else 0)


@pytest.mark.parametrize("row", PLAIN, ids=lambda r: "row%d" % r[0])
def test_route_table(exe, row):
    three = row[1][:9] + (3,) + row[1][10:]
    got = run(exe, [row[1], three])
    assert got[0] == expected(row, False), row[0]
    assert got[1] == expected(row, True), row[0] + 20
    assert got[1]["variant"] == routes.ROWS[row[0] + 20]


def test_blocksize_1_has_no_warm_up_costs_and_a_low_frame_fewer_rows(exe):
    one, low = run(exe, [cfg(D=16, bs=1, paths=3), cfg(D=16, H=3, bs=9, paths=3)])
    assert (one["variant"], one["warm"], one["wrows"], one["R"]) == ("bt8_fused", 0, 0, 0)
    assert (low["variant"], low["warm"], low["wrows"], low["R"]) == ("bt8_box_w3", 1, 3, 4)


def test_rows_are_numbered_in_order_and_named_apart():
    assert [r[0] for r in PLAIN] == list(range(1, 21)) and sorted(routes.ROWS) == list(range(1, 41))
    assert len(set(routes.ROWS.values())) == 40 and [routes.ROWS[r[0]] for r in PLAIN] == routes.PLAIN


def test_the_command_line_form_prints_the_same(exe):
    c = PLAIN[0][1]
    p = subprocess.run([exe] + [str(v) for v in c], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout == ("bt8_fused form=BT8 sum=FUSED R=3 records=8 volume=NONE check=0 limit=0 warm=0 wrows=0 "
                                              "ftz=15 cw=0 ch=0\n"), p.stdout + p.stderr
    assert subprocess.run([exe, "1", "2"], capture_output=True).returncode == 2


# ---- the model: the launches of the replaced branch nest, in order.  A launch is (kernel, records or volume it reads, what it
# writes, the scalar arguments that the route decides).  The three pixel-cost kernels carry the names of the template that
# replaced them (k_sgm_pix -> k_sgm_pix<Cost8>, k_sgm_pix_census -> <CostCensus>, k_sgm_pix16<CN> -> <Cost16<CN>>).
def model(D, H, bs, P2, cn, ftz, kind, cw, ch, paths, f16):
    census = kind == 1
    M = cw * ch - 1 if census else cn * (2 * ftz + 63)                    # sgm_cost_limit (api_sgm.hip)
    limit = 32767 - P2 if M * bs * bs + P2 > 32767 else 0
    Rw, dq = bs // 2, D // 4
    fused = Rw <= 3 and dq in (4, 8, 16, 32, 64)
    out = []

    def pixbox(F, rec, lim):
        out.append(("k_sgm_pixbox<%s,%d,%d>" % (F, Rw, dq), rec, "C", lim))

    def box(T, vol):                                                      # launch_box<T>
        rmax = 8 if T == "u8" else 6
        if Rw <= 8 and Rw <= rmax:
            out.append(("k_sgm_box<%d,%s>" % (Rw, T), vol, "C", limit))
        else:
            out.append(("k_sgm_box_any<%s>" % T, vol, "C", Rw, limit))

    need16 = cn != 1 or 2 * ftz + 63 > 255 or bool(f16)                   # sgm_cost16_needed
    if census:                                                            # launch_sgm_cost
        out.append(("k_sgm_census<%d,%d>" % ({3: 1, 5: 2, 7: 3}.get(cw, 4), {3: 1, 5: 2}.get(ch, 3)), "frames", "g"))
        if fused and not limit:
            pixbox("CostCensus", "g", 0)
        else:
            out.append(("k_sgm_pix<CostCensus>", "g", "pix"))
            box("u8", "pix")
    else:
        rec = "c" if cn == 3 else "g"
        out.append(("k_sgm_bounds<%d>" % (3 if cn == 3 else 1), "frames", rec, ftz))
        if not need16:
            if fused and not limit:
                pixbox("Cost8", rec, 0)
            else:
                out.append(("k_sgm_pix<Cost8>", rec, "pix"))
                box("u8", "pix")
        elif fused:
            pixbox("Cost16<3>" if cn == 3 else "Cost16<1>", rec, limit)
        else:
            out.append(("k_sgm_pix<%s>" % ("Cost16<3>" if cn == 3 else "Cost16<1>"), rec, "S"))
            box("u16", "S")
    if paths == 3 and Rw != 0:                                            # launch_sgm_warm3
        rec = "c" if not census and cn == 3 else "g"
        F = "CostCensus" if census else ("Cost8" if not need16 else ("Cost16<3>" if cn == 3 else "Cost16<1>"))
        out.append(("k_sgm_warm3<%s>" % F, rec, "Cw", Rw, min(bs // 2, H), limit))
    return limit, out


FORM_TYPE = {"BT8": "Cost8", "BT16_GRAY": "Cost16<1>", "BT16_COLOUR": "Cost16<3>", "CENSUS": "CostCensus"}


def issued(p, D):
    """the launches of the new launch_sgm_cost for a printed plan, in its order: it reads the plan and nothing else (D: the grid)"""
    F, rec = FORM_TYPE[p["form"]], {8: "g", 24: "c"}[p["records"]]
    T = "u16" if p["form"].startswith("BT16") else "u8"
    vol = {"PIX": "pix", "S": "S", "NONE": None}[p["volume"]]
    out = []
    if p["form"] == "CENSUS":
        out.append(("k_sgm_census<%d,%d>" % ({3: 1, 5: 2, 7: 3}.get(p["cw"], 4), {3: 1, 5: 2}.get(p["ch"], 3)), "frames", rec))
    else:
        out.append(("k_sgm_bounds<%d>" % (3 if p["records"] == 24 else 1), "frames", rec, p["ftz"]))
    if vol:
        out.append(("k_sgm_pix<%s>" % F, rec, vol))
    if p["sum"] == "FUSED":
        out.append(("k_sgm_pixbox<%s,%d,%d>" % (F, p["R"], D // 4), rec, "C", p["limit"]))
    elif p["sum"] == "BOX":
        out.append(("k_sgm_box<%d,%s>" % (p["R"], T), vol, "C", p["limit"]))
    else:
        out.append(("k_sgm_box_any<%s>" % T, vol, "C", p["R"], p["limit"]))
    if p["warm"]:
        out.append(("k_sgm_warm3<%s>" % F, rec, "Cw", p["R"], p["wrows"], p["limit"]))
    return out


def sweep_space():
    Ds = (16, 32, 48, 64, 80, 128, 256, 272, 512)            # inside and outside {16 .. 256}, above 256
    windows = tuple(range(1, 22)) + (255,)
    P2s = (601, 2400, 16000, 32000)                          # cost_limit zero and non-zero for every form
    for D, bs, P2, paths, H in itertools.product(Ds, windows, P2s, (3, 4, 5, 8), (5, 24)):
        for cn, ftz, f16 in itertools.product((1, 3), (15, 95, 96, 97, 127), (0, 1)):
            yield cfg(D=D, H=H, bs=bs, P2=P2, cn=cn, ftz=ftz, paths=paths, f16=f16)
        for census, f16 in itertools.product(CENSUS_WINDOWS, (0, 1)):
            yield cfg(D=D, H=H, bs=bs, P2=P2, census=census, paths=paths, f16=f16)


def test_the_model_agrees_with_the_route_table():
    for row in PLAIN:
        for warm in (False, True):
            c = row[1][:9] + (3 if warm else 5,) + row[1][10:]
            e = expected(row, warm)
            assert model(*c) == (e["limit"], issued(e, c[0])), row[0]


@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_the_program_equals_the_model_over_the_sweep(exe, exe_san, which):
    cfgs = list(sweep_space())
    got = run(exe if which == "plain" else exe_san, cfgs)    # (sanitized: a finding aborts the program and fails the run)
    seen, seen_even = set(), set()
    for c, p in zip(cfgs, got):
        limit, launches = model(*c)
        assert (p["limit"], issued(p, c[0])) == (limit, launches), c
        assert p["check"] == int(limit > 0) and p["R"] == c[2] // 2
        assert p["variant"] == "%s_%s%s%s" % ({"BT8": "bt8", "BT16_GRAY": "bt16g", "BT16_COLOUR": "bt16c", "CENSUS": "census"}[p["form"]],
                                             {"FUSED": "fused", "BOX": "box", "BOX_ANY": "any"}[p["sum"]],
                                             "_chk" if p["check"] else "", "_w3" if p["warm"] else ""), c
        (seen if c[2] % 2 else seen_even).add(p["variant"])
    # the table has a row for every combination the sweep reaches at the odd windows a handle can have, and no other; the even
    # window 18 (rtdm_sgm_create makes it 19) is the one place where BT8 sums over k_sgm_box_any without a check
    assert seen == set(routes.ROWS.values())
    assert seen_even - seen == {"bt8_any", "bt8_any_w3"}
    assert not (seen | seen_even) & {v + w for v in routes.UNREACHABLE for w in ("", "_w3")}


# ---- the device cases of sgm_cost_routes.py
def test_every_device_case_plans_to_the_route_its_row_names(exe):
    got = run(exe, [c.plan_numbers() for c in routes.CASES])
    for c, p in zip(routes.CASES, got):
        assert p["variant"] == routes.ROWS[c.row], c.name
        assert 12 <= c.H <= 24 and c.W - c.D == 21
    assert sorted({c.row for c in routes.CASES}) == list(range(1, 41))               # one case per row at the least
    assert len({c.name for c in routes.CASES}) == len(routes.CASES)
    # a frame too low for b.pix to hold C' (api_sgm.hip, sgm_warm_buffer: 3 frames of 3 stripes x wrows rows of u16 against W H D bytes)
    assert any(c.paths == 3 and 3 * 3 * min(c.bs // 2, c.H) * (c.W - c.D) * c.D * 2 > 3 * c.W * c.H * c.D for c in routes.CASES)
    for c in routes.CASES:
        if c.paths == 3:                                     # k_sgm_warm3 has rows to write: a stripe starts below row 0
            import sgm_3way_ref
            assert any(a > 0 and o < e for a, o, e in sgm_3way_ref.stripes(c.H, c.bs)), c.name


@pytest.mark.parametrize("case", routes.CASES, ids=lambda c: c.name)
def test_expected_frames_are_live_different_and_not_refused(oracle, case):
    want = [case.want(L, R, oracle) for L, R in case.frames()]                       # (a refused frame raises)
    assert all((w[:, case.D:] != -16).mean() > 0.25 for w in want), [float((w[:, case.D:] != -16).mean()) for w in want]
    assert len({w.tobytes() for w in want}) == 3
