"""The matcher's geometry header (rt-depth-map_amd/csrc/rtdm_bm_geom.h, rule B3 of DESIGN.md section 4.19) without a device:
tests/bm_geom_host.cpp, built with g++ plainly and with -fsanitize=address,undefined, runs bm_roi_rect over the ROI sets of
tests/bm_geom_cases.py -- inside the frame, cut by each edge, negative origins, narrower than the window, w or h <= 0, INT_MIN /
INT_MAX in every field -- for every configuration there, and must print what make_geom restated in Python integers gives, the
sanitizers silent.  tests/golden/bm_geom_make_geom.json pins the host's make_geom: its rows were recorded from the 32-bit
arithmetic the matcher used before the geometry moved into the header.  Then the refusals of the three new entry points that
need no device."""
import ctypes as C
import json
import os
import subprocess

import pytest

import bm_geom_cases as gc
from conftest import ROOT, load


@pytest.fixture(scope="module")
def build(tmp_path_factory):
    out = tmp_path_factory.mktemp("bm_geom_host")

    def make(sanitize):
        exe = str(out / ("geom_san" if sanitize else "geom"))
        flags = ["-fsanitize=undefined,address", "-fno-sanitize-recover=all", "-g"] if sanitize else []
        subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-Werror", *flags, "-I",
                               os.path.join(ROOT, "rt-depth-map_amd", "csrc"), os.path.join(ROOT, "tests", "bm_geom_host.cpp"), "-o", exe])
        return exe
    return make


def run_lines(exe, text):
    run = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", run.stderr[-2000:]
    return [tuple(int(v) for v in ln.split()) for ln in run.stdout.splitlines()]


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_header_agrees_with_python_integers_on_every_roi_set(build, sanitize):
    cases = gc.cases()
    got = run_lines(build(sanitize), gc.lines())
    assert len(got) == len(cases) >= 500
    for (cfg, roi, env, _), g in zip(cases, got):
        assert g == gc.rect(cfg, roi, env), (cfg, roi, env)


def test_envelope_holds_the_rectangle_of_every_roi():
    """what rtdm_bm_compute_device_rois searches once for the batch covers what every frame's own restricted search covers"""
    for cfg in gc.CONFIGS:
        ex0, ex1, ey0, ey1, ec0, ec1, eany = gc.rect(cfg, None, True)
        for roi, _ in gc.rois(cfg[0], cfg[1]):
            vx0, vx1, vy0, vy1, cx0, cx1, any_ = gc.rect(cfg, roi)
            if not any_:
                continue
            assert eany and ex0 <= vx0 and vx1 <= ex1 and ey0 <= vy0 and vy1 <= ey1 and ec0 <= cx0 and cx1 <= ec1, (cfg, roi)


def test_host_make_geom_gives_what_it_gave(build):
    rows = json.load(open(os.path.join(ROOT, "tests", "golden", "bm_geom_make_geom.json")))["rows"]
    assert len(rows) >= 200
    mine = set(gc.lines().splitlines())
    assert all(r["case"] in mine for r in rows)                  # the fixture's cases are still among the sweep's
    got = run_lines(build(True), "".join(r["case"] + "\n" for r in rows))
    assert got == [tuple(r["rect"]) for r in rows]


def test_refusals_that_need_no_device():
    B = load("binding")
    L = B.lib()
    one = C.c_int(5)
    buf = (C.c_int * 16)()
    p = C.addressof(buf)
    # RTDM_ERR_NULL comes first, before sizes and before any device use (B5)
    assert L.rtdm_bm_compute_device_rois(None, 1, p, p, 64, 64 * 48, 64, 48, p, p, 128, 128 * 48, None) == -7
    assert L.rtdm_bm_compute_device_rois(None, 0, None, None, 0, 0, 0, 0, None, None, 0, 0, None) == -7
    assert L.rtdm_estimator_set_device_roi(None, 1) == -7
    assert L.rtdm_estimator_get_device_roi(None, C.byref(one)) == -7 and one.value == 5
    assert "rtdm_bm_compute_device_rois" in B.EXPORTS and "rtdm_estimator_set_device_roi" in B.EXPORTS
