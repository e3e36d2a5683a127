"""What plan_sgm (rt-depth-map_amd/csrc/k_sgm.hip) plans for the path passes of a StereoSGBM call, through the stand-alone
program tests/sgm_plan_host.cpp: built with hipcc (host code only) into a temporary directory and linked against
librtdm_hip.so, which loads without a device.  ROUTES are the rows of DESIGN.md ("SGM: routes"), pass by pass; the model
below restates the schedule of the launcher that plan_sgm replaced (its loop over the directions with its `sweep`, `swept_*`
and `s2_pending` flags, its probe launch and its strip-width choice), and the program is swept against it."""
import itertools
import os
import random
import subprocess

import pytest

from conftest import PKG, ROOT

DIRS = [(1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, 1), (1, -1), (-1, -1)]
SWEEP_RING = 4
HOOKS = ("RTDM_SGM_SWEEP", "RTDM_SGM_DUAL", "RTDM_SGM_SWEEP_COLS")


def np2(D):
    return 1 if D <= 64 else (2 if D <= 128 else 4)


def ring_for(W1, n, D, cols=1):
    """the ring words that n frames of strips of 8 * cols columns need"""
    return n * ((W1 + 8 * cols - 1) // (8 * cols)) * 2 * SWEEP_RING * 32 * np2(D)


def caps(down0=4096, down1=4096, up0=4096, up1=4096):
    """[LAST][columns 1 / 2 / 4][ADD2]; each argument one number for the three widths or a triple"""
    t = lambda v: tuple(v) if isinstance(v, (tuple, list)) else (v, v, v)
    lo0, lo1, hi0, hi1 = t(down0), t(down1), t(up0), t(up1)
    return tuple(x for a, b in ((lo0, lo1), (hi0, hi1)) for c in range(3) for x in (a[c], b[c]))


class Cfg:
    def __init__(self, D=64, paths=8, W1=61, n=1, s2=1, sweep=1, ring=None, wide=0, done=(0, 0, 0), cap=None):
        self.D, self.paths, self.W1, self.n, self.s2, self.sweep, self.wide, self.done = D, paths, W1, n, s2, sweep, wide, done
        self.ring = ring_for(W1, n, D) if ring is None else ring
        self.cap = caps() if cap is None else cap

    def numbers(self):
        return [self.D, self.paths, self.W1, self.n, self.s2, self.sweep, self.ring, self.wide] + list(self.done) + list(self.cap)


# ---- expected passes, as the program prints them (without the variant)
def H(k, s2=0, last=0):
    return "PATH_H (%d,%d) first=%d last=%d s2=%d" % (DIRS[k][0], DIRS[k][1], k == 0, last, s2)


def V(dy, s2=0, last=0):
    return "VERT (0,%d) first=0 last=%d s2=%d" % (dy, last, s2)


def SW(dy, cols, strips, items, grid, s2=0, last=0):
    return "SWEEP (0,%d) first=0 last=%d s2=%d cols=%d strips=%d items=%d grid=%d" % (dy, last, s2, cols, strips, items, grid)


def WD(k, waves, last=0):
    return "WIDE (%d,%d) first=%d last=%d s2=0 waves=%d" % (DIRS[k][0], DIRS[k][1], k == 0, last, waves)


def V3(s2=0):
    return "VERT3 (0,1) first=0 last=1 s2=%d" % s2


ADD = "ADD_S2 (0,0) first=0 last=0 s2=0"

# W1 = 61: 8 / 4 / 2 strips of 8 / 16 / 32 columns.  (number of the row in DESIGN.md, configuration, hooks, variant, passes)
ROUTES = [
    (1, Cfg(paths=8), {}, "sweep", [H(0, s2=1), SW(1, 1, 8, 8, 8, s2=1), SW(-1, 1, 8, 8, 8, last=1)]),
    (2, Cfg(paths=5), {}, "sweep", [H(0, s2=1), SW(1, 1, 8, 8, 8, s2=1, last=1)]),
    (3, Cfg(paths=4, sweep=0, ring=0), {}, "vert", [H(0, s2=1), V(1, s2=1), V(-1, last=1)]),
    (4, Cfg(paths=8, s2=0), {}, "sweep", [H(0), H(1), SW(1, 1, 8, 8, 8), SW(-1, 1, 8, 8, 8, last=1)]),
    (5, Cfg(paths=5, s2=0), {}, "sweep", [H(0), H(1), SW(1, 1, 8, 8, 8, last=1)]),
    (6, Cfg(paths=4, s2=0, sweep=0, ring=0), {}, "vert", [H(0), H(1), V(1), V(-1, last=1)]),
    (7, Cfg(paths=8), {"RTDM_SGM_SWEEP": "0"}, "half", [H(k, last=k == 7) for k in range(8)]),
    (8, Cfg(paths=5), {"RTDM_SGM_SWEEP": "0"}, "half", [H(k, last=k == 5) for k in (0, 1, 2, 4, 5)]),
    (9, Cfg(paths=4, sweep=0, ring=0), {"RTDM_SGM_SWEEP": "0"}, "half", [H(k, last=k == 3) for k in range(4)]),
    (10, Cfg(paths=8), {"RTDM_SGM_DUAL": "0"}, "sweep", [H(0), H(1), SW(1, 1, 8, 8, 8), SW(-1, 1, 8, 8, 8, last=1)]),
    (11, Cfg(paths=5), {"RTDM_SGM_DUAL": "0"}, "sweep", [H(0), H(1), SW(1, 1, 8, 8, 8, last=1)]),
    (12, Cfg(paths=4, sweep=0, ring=0), {"RTDM_SGM_DUAL": "0"}, "vert", [H(0), H(1), V(1), V(-1, last=1)]),
    (13, Cfg(paths=8), {"RTDM_SGM_SWEEP_COLS": "1"}, "sweep", [H(0, s2=1), SW(1, 1, 8, 8, 8, s2=1), SW(-1, 1, 8, 8, 8, last=1)]),
    (14, Cfg(paths=8), {"RTDM_SGM_SWEEP_COLS": "2"}, "sweep", [H(0, s2=1), SW(1, 2, 4, 4, 4, s2=1), SW(-1, 2, 4, 4, 4, last=1)]),
    (15, Cfg(paths=8), {"RTDM_SGM_SWEEP_COLS": "4"}, "sweep", [H(0, s2=1), SW(1, 4, 2, 2, 2, s2=1), SW(-1, 4, 2, 2, 2, last=1)]),
    # capacity 5: no room for 8 strips of 8 columns, 4 of 16 fit; three frames: 6 strips of 32 on 4 workgroups, whole frames per round
    (16, Cfg(paths=8, cap=caps(5, 5, 5, 5)), {}, "sweep", [H(0, s2=1), SW(1, 2, 4, 4, 4, s2=1), SW(-1, 2, 4, 4, 4, last=1)]),
    (17, Cfg(paths=8, n=3, cap=caps(5, 5, 5, 5)), {}, "sweep", [H(0, s2=1), SW(1, 4, 2, 6, 4, s2=1), SW(-1, 4, 2, 6, 4, last=1)]),
    (18, Cfg(paths=8, cap=caps(5, 5, 5, 5)), {"RTDM_SGM_SWEEP_COLS": "1"}, "sweep",
     [H(0, s2=1), SW(1, 2, 4, 4, 4, s2=1), SW(-1, 2, 4, 4, 4, last=1)]),
    (19, Cfg(paths=8, cap=caps(3, 3, 3, 3)), {}, "sweep", [H(0, s2=1), SW(1, 4, 2, 2, 2, s2=1), SW(-1, 4, 2, 2, 2, last=1)]),
    # a ring of 4 strips' words: the pick (8 columns, 8 strips) does not fit it, 16 columns do
    (20, Cfg(paths=8, ring=ring_for(61, 1, 64, 2)), {}, "sweep", [H(0, s2=1), SW(1, 2, 4, 4, 4, s2=1), SW(-1, 2, 4, 4, 4, last=1)]),
    (21, Cfg(paths=8, cap=caps(4096, 4096, 1, 1)), {}, "sweep", [H(0, s2=1), SW(1, 1, 8, 8, 8, s2=1), H(3), H(6), H(7, last=1)]),
    (22, Cfg(paths=8, cap=caps(4096, 1, 4096, 4096)), {}, "sweep", [H(0), H(1), SW(1, 1, 8, 8, 8), SW(-1, 1, 8, 8, 8, last=1)]),
    (23, Cfg(paths=8, sweep=0), {}, "half", [H(k, last=k == 7) for k in range(8)]),
    (24, Cfg(paths=5, cap=caps(1, 1, 1, 1)), {}, "half", [H(k, last=k == 5) for k in (0, 1, 2, 4, 5)]),
    (25, Cfg(D=272, paths=8, s2=0, sweep=0), {}, "wide_w1", [WD(k, 1, last=k == 7) for k in range(8)]),
    (26, Cfg(D=1040, paths=5, s2=0, sweep=0), {}, "wide_w4", [WD(k, 4, last=k == 5) for k in (0, 1, 2, 4, 5)]),
    (27, Cfg(paths=8, wide=1), {"RTDM_SGM_SWEEP": "0"}, "wide_w1", [WD(k, 1, last=k == 7) for k in range(8)]),
    (28, Cfg(paths=4, wide=4, sweep=0, ring=0), {}, "wide_w4", [WD(k, 4, last=k == 3) for k in range(4)]),
    # the remainder of a call whose sweep the runtime refused: down with S2 pending / not, MODE_SGBM's down, up
    (29, Cfg(paths=8, sweep=0, done=(0b11, 1, 0)), {}, "half", [ADD] + [H(k, last=k == 7) for k in range(2, 8)]),
    (30, Cfg(paths=8, s2=0, sweep=0, done=(0b11, 0, 0)), {}, "half", [H(k, last=k == 7) for k in range(2, 8)]),
    (31, Cfg(paths=5, sweep=0, done=(0b11, 1, 0)), {}, "half", [ADD, H(2), H(4), H(5, last=1)]),
    (32, Cfg(paths=8, sweep=0, done=(0b00110111, 0, 1)), {}, "sweep", [H(3), H(6), H(7, last=1)]),
    # MODE_SGBM_3WAY: with S2, without it or under RTDM_SGM_DUAL=0 (two configurations of row 34), and under the hook and the
    # debug switch that it does not consult (two of row 35)
    (33, Cfg(paths=3), {}, "vert3", [H(0, s2=1), V3(s2=1)]),
    (34, Cfg(paths=3, s2=0), {}, "vert3", [H(0), H(1), V3()]),
    (34, Cfg(paths=3), {"RTDM_SGM_DUAL": "0"}, "vert3", [H(0), H(1), V3()]),
    (35, Cfg(paths=3), {"RTDM_SGM_SWEEP": "0"}, "vert3", [H(0, s2=1), V3(s2=1)]),
    (35, Cfg(paths=3, wide=4, sweep=0, ring=0), {}, "vert3", [H(0, s2=1), V3(s2=1)]),
]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("sgm_plan") / "sgm_plan_host")
    lib = os.path.join(ROOT, PKG, "lib")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, PKG, "csrc"),
                           os.path.join(ROOT, "tests", "sgm_plan_host.cpp"), "-L" + lib, "-lrtdm_hip", "-Wl,-rpath," + lib, "-o", out])
    return out


def run(exe, cfgs, hooks=None):
    """-> per configuration (variant, [pass lines without the variant]); the configurations travel on standard input"""
    e = {k: v for k, v in os.environ.items() if k not in HOOKS}
    e.update(hooks or {})
    text = "".join(" ".join(str(v) for v in c.numbers()) + "\n" for c in cfgs)
    p = subprocess.run([exe, "-"], input=text, capture_output=True, text=True, env=e)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    out, cur = [], []
    for line in p.stdout.splitlines():
        if line == "end":
            variants = {ln.split(" ", 1)[0] for ln in cur}
            assert len(variants) == 1, cur
            out.append((variants.pop(), [ln.split(" ", 1)[1] for ln in cur]))
            cur = []
        else:
            cur.append(line)
    assert not cur and len(out) == len(cfgs)
    return out


def test_the_command_line_form_prints_the_same(exe):
    c = ROUTES[0][1]
    p = subprocess.run([exe] + [str(v) for v in c.numbers()], capture_output=True, text=True,
                       env={k: v for k, v in os.environ.items() if k not in HOOKS})
    assert p.returncode == 0 and p.stdout.splitlines() == ["sweep " + ln for ln in ROUTES[0][4]] + ["end"], p.stdout + p.stderr
    assert subprocess.run([exe, "1", "2"], capture_output=True).returncode == 2


@pytest.mark.parametrize("row", ROUTES, ids=["row%d%s" % (r[0], "b" if i and ROUTES[i - 1][0] == r[0] else "") for i, r in enumerate(ROUTES)])
def test_route_table(exe, row):
    num, cfg, hooks, variant, passes = row
    assert run(exe, [cfg], hooks) == [(variant, passes)], num


def test_route_rows_are_numbered_in_order_and_fit_a_plan():
    nums = [r[0] for r in ROUTES]                         # (rows 34 and 35 name two configurations each)
    assert nums == sorted(nums) and sorted(set(nums)) == list(range(1, 36))
    assert all(1 <= len(r[4]) <= 8 for r in ROUTES)


# ---- the model: the launcher that plan_sgm replaced, restated.  `refuse`: the sweep ("down" / "up") whose launch the runtime
# refuses (a launch that passed every check and then returned "not launched").
def model_sweep(c, hooks, last, add2, probe=False, refused=False):
    """the strip-width dispatcher and the per-width launcher up to the launch -> (cols, strips, items, grid) or None"""
    cap = lambda cols: c.cap[(last * 3 + {1: 0, 2: 1, 4: 2}[cols]) * 2 + add2]
    cols_env = int(hooks.get("RTDM_SGM_SWEEP_COLS", 0))
    pick = cols_env if cols_env else (1 if c.n * ((c.W1 + 7) // 8) <= cap(1) else (2 if c.n * ((c.W1 + 15) // 16) <= cap(2) else 4))

    def one(cols):
        strips = (c.W1 + 8 * cols - 1) // (8 * cols)
        if cap(cols) < strips:
            return None
        items = c.n * strips
        if items * 2 * SWEEP_RING * 32 * np2(c.D) > c.ring:
            return None
        if probe:
            return True
        if refused:
            return None
        return (cols, strips, items, items if items <= cap(cols) else cap(cols) // strips * strips)

    if pick == 1:
        r = one(1)
        if r:
            return r
    if pick <= 2:
        r = one(2)
        if r:
            return r
    return one(4)


def model(c, hooks, refuse=None):
    """-> (variant, passes) of a whole call"""
    if c.paths == 3:
        # MODE_SGBM_3WAY (newer than the launcher restated below): the horizontal pair as for
        # MODE_HH4, then the striped downward pass; no sweep, no wide form, RTDM_SGM_DUAL = 0 keeps its meaning
        dual = bool(int(hooks.get("RTDM_SGM_DUAL", 1)) and c.s2)
        return "vert3", [H(0, s2=dual)] + ([] if dual else [H(1)]) + [V3(s2=dual)]
    last_dir = {4: 3, 5: 5, 8: 7}[c.paths]
    if c.D > 256 or c.wide:
        waves = 4 if (c.wide == 4 or c.D > 1024) else 1
        return "wide_w%d" % waves, [WD(k, waves, last=k == last_dir) for k in range(last_dir + 1) if not (c.paths == 5 and DIRS[k][1] < 0)]
    sweep_env, dual_env = int(hooks.get("RTDM_SGM_SWEEP", 1)), int(hooks.get("RTDM_SGM_DUAL", 1))
    sweep = bool(sweep_env and c.sweep)
    out = []
    if c.paths == 4:
        if not sweep_env:
            return "half", [H(k, last=k == 3) for k in range(4)]
        dual = bool(dual_env and c.s2)
        out.append(H(0, s2=dual))
        if not dual:
            out.append(H(1))
        return "vert", out + [V(1, s2=dual), V(-1, last=1)]
    swept_down = swept_up = s2_pending = swept = False
    for k in range(8):
        dx, dy = DIRS[k]
        if c.paths == 5 and dy < 0:
            continue
        if k == 0 and sweep and dual_env and c.s2 and model_sweep(c, hooks, c.paths == 5, 1, probe=True):
            out.append(H(0, s2=1))
            s2_pending = True
            continue
        if k == 1 and s2_pending:
            continue
        if dy != 0:
            if swept_down if dy > 0 else swept_up:
                continue
            if sweep and k in (2, 3):
                last_sweep = c.paths == 5 or dy < 0
                r = model_sweep(c, hooks, last_sweep, int(s2_pending), refused=refuse == ("down" if dy > 0 else "up"))
                if r:
                    out.append(SW(dy, *r, s2=int(s2_pending), last=int(last_sweep)))
                    if dy > 0:
                        swept_down = True
                    else:
                        swept_up = True
                    s2_pending = False
                    swept = True
                    continue
                sweep = False
            if s2_pending:
                out.append(ADD)
                s2_pending = False
        out.append(H(k, last=k == last_dir))
    return ("sweep" if swept else "half"), out


def test_the_model_agrees_with_the_route_table():
    for num, cfg, hooks, variant, passes in ROUTES:
        if cfg.done == (0, 0, 0):
            assert model(cfg, hooks) == (variant, passes), num


def done_after(passes):
    """what the launcher hands plan_sgm after these passes of a plan: (direction bits, S2 pending, a sweep ran)"""
    dirs, pending, swept = 0, 0, 0
    for ln in passes:
        kind, d = ln.split(" ")[0], ln.split(" ")[1]
        if kind == "ADD_S2":
            pending = 0
            continue
        k = DIRS.index(tuple(int(v) for v in d.strip("()").split(",")))
        dirs |= 1 << k
        if kind == "PATH_H" and ln.split(" ")[4] == "s2=1":
            dirs |= 2
            pending = 1
        if kind == "SWEEP":
            dirs |= 0x30 if k == 2 else 0xc0
            pending, swept = 0, 1
    return dirs, pending, swept


def sweep_space(rng):
    for D, paths, W1, n, s2 in itertools.product((16, 64, 80, 128, 256, 272, 1024, 1040), (4, 5, 8), (1, 7, 8, 9, 34, 61, 1216),
                                                 (1, 3, 16), (0, 1)):
        # each capacity at each value: every uniform table, and tables with each of the twelve drawn on its own
        tables = [caps(v, v, v, v) for v in (-1, 1, 5, 160, 4096)] + [tuple(rng.choice((-1, 1, 5, 160, 4096)) for _ in range(12)) for _ in range(5)]
        for cap in tables:
            # a ring that holds the 8-column strips of the call, and one that holds 16-column strips only
            for ring in (ring_for(W1, n, D, 1), ring_for(W1, n, D, 2)):
                yield Cfg(D=D, paths=paths, W1=W1, n=n, s2=s2 if D <= 256 else 0, sweep=int(paths != 4 and D <= 256), ring=ring, cap=cap)


@pytest.mark.parametrize("hooks", [{}, {"RTDM_SGM_SWEEP": "0"}, {"RTDM_SGM_DUAL": "0"}, {"RTDM_SGM_SWEEP_COLS": "1"},
                                   {"RTDM_SGM_SWEEP_COLS": "2"}, {"RTDM_SGM_SWEEP_COLS": "4"}],
                         ids=lambda h: "_".join("%s%s" % (k[9:], v) for k, v in h.items()) or "default")
def test_the_program_equals_the_model_over_the_sweep(exe, hooks):
    cfgs = list(sweep_space(random.Random(20)))
    got = run(exe, cfgs, hooks)
    kinds = set()
    refused = []                       # (whole-call configuration, which sweep, passes before it, the replan's configuration)
    for c, g in zip(cfgs, got):
        assert g == model(c, hooks), (c.numbers(), hooks)
        kinds.update(ln.split(" ")[0] for ln in g[1])
        for i, ln in enumerate(g[1]):
            if ln.startswith("SWEEP"):
                r = Cfg(D=c.D, paths=c.paths, W1=c.W1, n=c.n, s2=c.s2, sweep=0, ring=c.ring, cap=c.cap, done=done_after(g[1][:i]))
                refused.append((c, "down" if "(0,1)" in ln else "up", g[1][:i], r))
    # a sweep that the runtime refuses: the passes before it and the plan of the remainder are what the old launcher went on with
    for (c, which, before, r), (variant, rest) in zip(refused, run(exe, [r for _, _, _, r in refused], hooks)):
        assert (variant, before + rest) == model(c, hooks, refuse=which), (c.numbers(), hooks, which)
        kinds.update(ln.split(" ")[0] for ln in rest)
    if not hooks:
        assert kinds == {"WIDE", "PATH_H", "VERT", "SWEEP", "ADD_S2"} and refused
    # the forced wide forms consult no hook and no limit
    wide = [Cfg(D=c.D, paths=c.paths, W1=c.W1, n=c.n, s2=c.s2, sweep=c.sweep, ring=c.ring, cap=c.cap, wide=w) for c in cfgs[::97] for w in (1, 4)]
    for c, g in zip(wide, run(exe, wide, hooks)):
        assert g == model(c, hooks), (c.numbers(), hooks)
