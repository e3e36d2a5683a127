"""Every route of the StereoSGBM path passes on pairs that reach the cases the kernels are built around (tests/sgm_hostile.py:
some but not all aggregated costs saturated, the overflow rule on its boundary, tied minima in different lanes, rows and waves,
tied votes, winners on both ends of the range, the disp12MaxDiff boundary), bit for bit against the oracle -- MODE_HH4 against
sgm_hh4_ref, colour and preFilterCap against sgm_cn_ref.  tests/test_sgm_hostile_cpu.py shows on the CPU that the pairs do what
they claim at the seeds and parameters of tests/sgm_hostile_cases.py.

Routes without a hook run in this process, each frame through `compute` (n = 1) and three through `compute_device`; the forced
forms (rtdm_debug_sgm_wide_paths, rtdm_debug_sgm_cost16) must give the narrow form's bytes; RTDM_SGM_SWEEP=0 ("half"),
RTDM_SGM_DUAL=0 and RTDM_SGM_SWEEP_COLS=2 / 4 are read once per process and run in one child process each."""
import contextlib
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import sgm_hostile as sh
import sgm_hostile_ref as hr
import sgm_hostile_cases as hc
from conftest import ROOT, load

pytestmark = pytest.mark.gpu

N = 3
SWEEPS = {8: 2, 5: 1, 4: 0}                                       # row-synchronous sweeps per call of the narrow default forms


@pytest.fixture(scope="module")
def pkg():
    import torch                         # torch first: it brings its own HIP runtime and must initialise before ours
    assert torch.cuda.is_available(), "the -m gpu suite needs an MI355X"
    return load()


def route(D, paths):
    """-> (variant, sweeps per call) of the default form"""
    if D > 1024:
        return "wide_w4", 0
    if D > 256:
        return "wide_w1", 0
    return ("vert" if paths == 4 else "sweep"), SWEEPS[paths]


@contextlib.contextmanager
def forced(pkg, wide=0, cost16=0):
    lib = pkg.binding.lib()
    try:
        lib.rtdm_debug_sgm_wide_paths(wide)
        lib.rtdm_debug_sgm_cost16(cost16)
        yield
    finally:
        lib.rtdm_debug_sgm_wide_paths(0)
        lib.rtdm_debug_sgm_cost16(0)


@functools.lru_cache(maxsize=None)
def frames(family, D, minD=0, seed=None):
    W1, H = hc.shape(D)
    L, R = sh.make_n(family, hc.seed(family, D) if seed is None else seed, N, hc.width(D, minD, W1), H, D, minD)
    L.setflags(write=False); R.setflags(write=False)
    return L, R


@functools.lru_cache(maxsize=None)
def expected(family, D, paths, k=0, minD=0, extra=(), seed=None):
    """-> (keywords, the reference's maps of the three frames): computed once, shared, read-only"""
    Ls, Rs = frames(family, D, minD, seed)
    kw = dict(hr.resolve(hc.param_sets(family, paths)[k], Ls, Rs, D, minD), **dict(extra))
    want = np.stack([hr.reference(L, R, paths, kw) for L, R in zip(Ls, Rs)])
    want.setflags(write=False)
    return kw, want


def matcher(pkg, kw, W, H, paths, n=N, cap=0):
    kw = dict(kw)
    kw["numOfDisparities"] = kw.pop("numDisparities")
    return pkg.HIPSemiGlobalMatcher(width=W, height=H, max_batch=n, paths=paths, preFilterCap=cap, **kw)


def device_maps(m, Ls, Rs):
    import torch
    dD = torch.full(Ls.shape[:3], 12345, dtype=torch.int16, device="cuda")
    m.compute_device(torch.from_numpy(np.array(Ls)).cuda(), torch.from_numpy(np.array(Rs)).cuda(), dD, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return dD.cpu().numpy()


def assert_same(got, want, what):
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError("%s: %d / %d pixels differ; first at (y,x)=%s got %d want %d" % (
            what, len(bad), got.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])]))


def run_case(pkg, family, D, paths, k=0, minD=0, extra=(), seed=None, variant=None, sweeps=None):
    """Frame `seed` through compute, frames seed .. seed + 2 through compute_device on the same handle; the path variant and the
    sweep count must be the route's (no test runs another kernel silently).  -> (the host call's map, the three maps, message)"""
    Ls, Rs = frames(family, D, minD, seed)
    kw = dict(hr.resolve(hc.param_sets(family, paths)[k], Ls, Rs, D, minD), **dict(extra))
    if variant is None:
        variant, sweeps = route(D, paths)
    H, W = Ls.shape[1:]
    m = matcher(pkg, kw, W, H, paths)
    try:
        one = m.compute(Ls[0], Rs[0])
        seen = [(m.path_variant, m.pass_stats())]
        three = device_maps(m, Ls, Rs)
        seen.append((m.path_variant, m.pass_stats()))
    finally:
        m.close()
    what = "%s seed %d D=%d paths=%d %dx%d minD=%d %s variant=%s" % (
        family, hc.seed(family, D) if seed is None else seed, D, paths, W, H, minD, kw, seen[0][0])
    assert seen == [(variant, ((i + 1) * sweeps, False)) for i in range(2)], "%s: ran %s" % (what, seen)
    return one, three, what


def check(pkg, family, D, paths, k=0, minD=0, extra=(), seed=None, variant=None, sweeps=None):
    """run_case, each frame against its own reference.  -> the three maps"""
    one, three, what = run_case(pkg, family, D, paths, k, minD, extra, seed, variant, sweeps)
    want = expected(family, D, paths, k, minD, extra, seed)[1]
    assert_same(one, want[0], what + " n=1")
    for i in range(N):
        assert_same(three[i], want[i], what + " n=3 frame %d" % i)
    return three


_OWN = {}


def own_maps(pkg, family, D, paths, k):
    """the default route's maps of this process, computed (and checked) once"""
    key = (family, D, paths, k)
    if key not in _OWN:
        _OWN[key] = check(pkg, family, D, paths, k)
    return _OWN[key]


def every_family(pkg, D, paths, families=sh.FAMILIES, **kw):
    for family in families:
        for k in range(len(hc.param_sets(family, paths))):
            check(pkg, family, D, paths, k, **kw)


ROUTES = [(D, p) for D in hc.NARROW_D + hc.WIDE_D for p in hc.MODES]
ROUTE_IDS = ["D%d-paths%d" % r for r in ROUTES]


# ---- 1. the routes a handle reaches without a hook ------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,paths", ROUTES, ids=ROUTE_IDS)
def test_every_family_on_every_route(pkg, oracle, D, paths):
    every_family(pkg, D, paths)
    kw, want = expected("partial_sat", D, paths)
    assert (want != -16).any() and len({w.tobytes() for w in want}) == N        # live frames, all different


@pytest.mark.parametrize("D,paths", ROUTES, ids=ROUTE_IDS)
def test_pins_on_their_live_boundaries(pkg, oracle, D, paths):
    assert hc.pins(D, paths)
    for family, _, _, seed, u in hc.pins(D, paths):
        a = check(pkg, family, D, paths, extra=(("uniquenessRatio", u),), seed=seed)
        b = check(pkg, family, D, paths, extra=(("uniquenessRatio", u + 1),), seed=seed)
        assert (a[0] != b[0]).any()
    maps = [check(pkg, "steps", D, paths, extra=(("disp12MaxDiff", v),)) for v in (-1, 0, 1, 2)]
    assert maps[0].tobytes() == maps[1].tobytes() == maps[2].tobytes()
    assert all(int((maps[2][i] != maps[3][i]).sum()) >= 10 for i in range(N))


@pytest.mark.parametrize("minD", (3, -5))
@pytest.mark.parametrize("D,paths", ROUTES, ids=ROUTE_IDS)
def test_min_disparity_on_every_route(pkg, oracle, D, paths, minD):
    # (minD = 0 is test_every_family_on_every_route; minD = 3: R9's scaled invalid vote is ">= minD", test_sgm_hostile_cpu)
    every_family(pkg, D, paths, ("ends", "steps", "vote_ties"), minD=minD)


# ---- 2. forced forms give the narrow form's bytes ---------------------------------------------------------------------------------------
FORCED_FAMILIES = ("ties", "ties35", "partial_sat", "at_limit")


@pytest.mark.parametrize("paths", hc.MODES)
@pytest.mark.parametrize("D", (64, 256))
@pytest.mark.parametrize("mode,variant", [(1, "wide_w1"), (4, "wide_w4")])
def test_forced_wide_lines(pkg, oracle, mode, variant, D, paths):
    for family in FORCED_FAMILIES:
        for k in range(len(hc.param_sets(family, paths))):
            narrow = own_maps(pkg, family, D, paths, k)
            with forced(pkg, wide=mode):
                wide = check(pkg, family, D, paths, k, variant=variant, sweeps=0)
            assert wide.tobytes() == narrow.tobytes(), (family, k)


@pytest.mark.parametrize("paths", hc.MODES)
@pytest.mark.parametrize("D", (64, 256, 48))
def test_forced_16_bit_cost_forms(pkg, oracle, D, paths):
    # (nothing the ABI reports separates the u8 from the u16 cost forms -- path_variant and pass_stats name the path passes only --
    # so this leg cannot tell whether the switch took effect, as in test_gpu_sgm_hh4.py; the colour and ftzero 97 cases of the
    # overflow boundary below reach the u16 forms without the switch)
    for family in FORCED_FAMILIES:
        for k in range(len(hc.param_sets(family, paths))):
            u8 = own_maps(pkg, family, D, paths, k)
            with forced(pkg, cost16=1):
                u16 = check(pkg, family, D, paths, k)
            assert u16.tobytes() == u8.tobytes(), (family, k)


# ---- 3. the overflow boundary ---------------------------------------------------------------------------------------------------------
def natural_pair(seed, W, H, shift, cn=1):
    """A smooth low-contrast pair (block costs far below the limit), gray or colour"""
    rng = np.random.default_rng(seed)
    T = rng.integers(0, 256, (H, W + shift, cn)).astype(np.float64)
    T = (T + np.roll(T, 1, 1) + np.roll(T, -1, 1) + np.roll(T, 1, 0) + np.roll(T, -1, 0)) / 5
    T = (T / 16).astype(np.uint8)
    L, R = T[:, :W].copy(), T[:, shift:shift + W].copy()
    return (L[:, :, 0].copy(), R[:, :, 0].copy()) if cn == 1 else (L, R)


def boundary(pkg, D, paths, cap=0, cn=1):
    """at_limit's first frame: accepted and right at P2 = 32767 - its largest block cost, refused at P2 + 1, and the handle that
    refused it serves a natural pair.  -> the variant of the accepted call"""
    W1, H = hc.shape(D)
    W = hc.width(D, 0, W1)
    seed = hc.seed("at_limit", D)
    L, R = sh.make("at_limit", seed, W, H, D)
    if cn == 3:
        L, R = sh.colour(L, R, seed)
    kw = hr.resolve(hc.AT_LIMIT, L[None], R[None], D, 0, cap)
    what = "at_limit seed %d D=%d paths=%d cap=%d cn=%d %s" % (seed, D, paths, cap, cn, kw)
    assert kw["P1"] < kw["P2"] <= 32000, what
    want = hr.reference(L, R, paths, kw, cap)
    with pytest.raises(ValueError):
        hr.reference(L, R, paths, dict(kw, P2=kw["P2"] + 1), cap)
    m = matcher(pkg, kw, W, H, paths, 1, cap)
    try:
        got, variant = m.compute(L, R), m.path_variant
    finally:
        m.close()
    assert_same(got, want, what + " variant=" + variant)
    assert (want != -16).sum() >= 0.3 * W1 * H, what                       # (of the cost domain)
    over = dict(kw, P2=kw["P2"] + 1)
    m = matcher(pkg, over, W, H, paths, 1, cap)
    try:
        with pytest.raises(pkg.binding.RtdmError) as e:
            m.compute(L, R)
        assert e.value.status == -6, what
        Ln, Rn = natural_pair(seed, W, H, 5, cn)
        assert_same(m.compute(Ln, Rn), hr.reference(Ln, Rn, paths, over, cap), what + " (a natural pair after the refusal)")
        assert m.path_variant == variant
    finally:
        m.close()
    return variant


@pytest.mark.parametrize("D,paths,variant", [(64, 8, "sweep"), (64, 5, "sweep"), (64, 4, "vert"), (272, 8, "wide_w1"), (1040, 5, "wide_w4")])
def test_overflow_boundary(pkg, oracle, D, paths, variant):
    assert boundary(pkg, D, paths) == variant


def test_overflow_boundary_16_bit_costs(pkg, oracle):
    with forced(pkg, cost16=1):
        assert boundary(pkg, 64, 5) == "sweep"


@pytest.mark.parametrize("cap,cn,paths", [(95, 1, 8), (97, 1, 5), (0, 3, 8), (63, 3, 4)],
                         ids=["u8-ftzero95", "u16-ftzero97", "colour", "colour-ftzero63-hh4"])
def test_overflow_boundary_prefilter_cap_and_colour(pkg, oracle, cap, cn, paths):
    boundary(pkg, 64, paths, cap, cn)


# ---- 4. hooked routes, one child process each -------------------------------------------------------------------------------------------
CHILD_D = (64, 128)
CHILD = r"""
import importlib, json, os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import numpy as np
import torch
assert torch.cuda.is_available()
pkg = importlib.import_module("rt-depth-map_amd")
import sgm_hostile as sh
import sgm_hostile_cases as hc
import test_gpu_sgm_hostile as T
variants = dict(zip(hc.MODES, json.loads(sys.argv[3])))
out = {}
for D in T.CHILD_D:
    for paths in hc.MODES:
        variant, sweeps = variants[paths]
        for family in sh.FAMILIES:
            for k in range(len(hc.param_sets(family, paths))):
                one, three, _ = T.run_case(pkg, family, D, paths, k, variant=variant, sweeps=sweeps)     # (the parent compares)
                out["%d_%d_%s_%d" % (D, paths, family, k)] = np.concatenate([one[None], three])
        if D == 64:
            out["boundary_%d" % paths] = np.array(T.boundary(pkg, D, paths))
np.savez(sys.argv[2], **out)
"""
HOOKS = [
    ({"RTDM_SGM_SWEEP": "0"}, {8: ("half", 0), 5: ("half", 0), 4: ("half", 0)}),
    ({"RTDM_SGM_DUAL": "0"}, {8: ("sweep", 2), 5: ("sweep", 1), 4: ("vert", 0)}),
    ({"RTDM_SGM_SWEEP_COLS": "2"}, {8: ("sweep", 2), 5: ("sweep", 1), 4: ("vert", 0)}),
    ({"RTDM_SGM_SWEEP_COLS": "4"}, {8: ("sweep", 2), 5: ("sweep", 1), 4: ("vert", 0)}),
]


@pytest.mark.parametrize("env,variants", HOOKS, ids=["%s=%s" % next(iter(h[0].items())) for h in HOOKS])
def test_hooked_routes_in_a_child_process(pkg, oracle, tmp_path, env, variants):
    script = tmp_path / "child.py"
    script.write_text(CHILD)
    out = tmp_path / "maps.npz"
    # (a child takes about 3.5 s on an MI355X, most of it the import of torch)
    r = subprocess.run([sys.executable, str(script), ROOT, str(out), json.dumps([variants[p] for p in hc.MODES])],
                       env=dict(os.environ, **env), capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    z = np.load(out)
    for D in CHILD_D:
        for paths in hc.MODES:
            for family in sh.FAMILIES:
                for k in range(len(hc.param_sets(family, paths))):
                    what = "%s %s D=%d paths=%d set %d" % (env, family, D, paths, k)
                    theirs = z["%d_%d_%s_%d" % (D, paths, family, k)]
                    want = expected(family, D, paths, k)[1]
                    assert_same(theirs[0], want[0], what + " n=1 (child against the reference)")
                    assert_same(theirs[1:], want, what + " n=3 (child against the reference)")
                    assert_same(theirs[1:], own_maps(pkg, family, D, paths, k), what + " (child against this process)")
    assert [str(z["boundary_%d" % p]) for p in hc.MODES] == [variants[p][0] for p in hc.MODES]
