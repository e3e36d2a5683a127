"""close() of the nine handle classes, which they share through the one Handle base: it frees the handle once, a second
close() and the drop of the last reference after it do nothing, and none of them raises.  No call is made on a closed handle.
64 x 48 frames, D = 16, blockSize 5; the rectifier comes from the 320x240 calibration files (crop 233x156), and the estimator
borrows it with a matcher and a detector of the crop's size."""
import sys

import numpy as np
import pytest

import calib_hostbuild as hb

pytestmark = pytest.mark.gpu

W, H = 64, 48
YML = hb.yml("320x240", "intrinsics"), hb.yml("320x240", "extrinsics")


@pytest.fixture(scope="module")
def pkg():
    import torch                         # torch first: it brings its own HIP runtime and must initialise before ours
    assert torch.cuda.is_available()
    from conftest import load
    return load()


@pytest.fixture
def unraisable(monkeypatch):
    """what a __del__ raised: Python reports it to this hook and goes on"""
    seen = []
    monkeypatch.setattr(sys, "unraisablehook", seen.append)
    return seen


def wls_filter(pkg):
    m = pkg.HIPMatcher(numOfDisparities=16, blockSize=5, width=W, height=H)
    f = pkg.create_disparity_wls_filter(m)
    m.close()
    return f


MAKERS = {
    "HIPMatcher": lambda pkg: pkg.HIPMatcher(numOfDisparities=16, blockSize=5, width=W, height=H),
    "HIPSemiGlobalMatcher": lambda pkg: pkg.HIPSemiGlobalMatcher(numOfDisparities=16, blockSize=5, width=W, height=H),
    "HIPDisparityWLSFilter": wls_filter,
    "HIPReprojector": lambda pkg: pkg.HIPReprojector(np.eye(4), W, H),
    "HIPMorphologicalFilter": lambda pkg: pkg.HIPMorphologicalFilter(W, H),
    "HIPRectifier": lambda pkg: pkg.HIPRectifier.from_calibration(*YML),
    "HIPMJPEGDecoder": lambda pkg: pkg.HIPMJPEGDecoder(W, H),
    "HIPObjectDetector": lambda pkg: pkg.HIPObjectDetector(W, H),
}


def close_twice(h):
    assert h._h
    h.close()
    assert h._h is None
    h.close()
    assert h._h is None


@pytest.mark.parametrize("name", sorted(MAKERS))
def test_close_twice_then_drop(pkg, unraisable, name):
    h = MAKERS[name](pkg)
    assert type(h) is getattr(pkg, name)
    close_twice(h)
    del h
    assert unraisable == []


def test_estimator_closes_before_the_handles_it_borrows(pkg, unraisable):
    rect = pkg.HIPRectifier.from_calibration(*YML)
    rw, rh = rect.roi[2], rect.roi[3]
    m = pkg.HIPMatcher(numOfDisparities=16, blockSize=5, width=rw, height=rh)
    det = pkg.HIPObjectDetector(rw, rh)
    est = pkg.HIPEstimator(m, rect, det)
    close_twice(est)
    del est
    for h in (det, m, rect):
        close_twice(h)
    del h, det, m, rect
    assert unraisable == []
