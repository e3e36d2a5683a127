"""Host builds of the calibration mathematics (rt-depth-map_amd/csrc/rtdm_calib.h) for the CPU tests: tests/calib_host.cpp
compiled with g++, plainly and with -fsanitize=address,undefined, once per test run into a temporary directory that is removed
when the interpreter exits; and the parser of what the program prints (doubles as hex floats)."""
import atexit
import os
import shutil
import subprocess
import tempfile

import numpy as np

from conftest import ROOT

CSRC = os.path.join(ROOT, "rt-depth-map_amd", "csrc")
YML = os.path.join(ROOT, "tests", "golden", "calib_yml")
RESOLUTIONS = ("320x240", "640x480", "1280x720")
_BUILT = {}


def yml(res, which):
    return os.path.join(YML, res, which + ".yml")


def tmpdir():
    if "dir" not in _BUILT:
        _BUILT["dir"] = tempfile.mkdtemp(prefix="calib_host_")
        atexit.register(shutil.rmtree, _BUILT["dir"], ignore_errors=True)
    return _BUILT["dir"]


def build_host(sanitize=False):
    key = "host_san" if sanitize else "host"
    if key not in _BUILT:
        exe = os.path.join(tmpdir(), key)
        flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
        subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-Werror", *flags, "-I", CSRC,
                               os.path.join(ROOT, "tests", "calib_host.cpp"), "-o", exe])
        _BUILT[key] = exe
    return _BUILT[key]


def run_host(*args, sanitize=False):
    """-> the process and what it printed as {name: float64 array | int tuple}; 'status' lines of the fuzz mode as a dict"""
    run = subprocess.run([build_host(sanitize), *[str(a) for a in args]], capture_output=True, text=True)
    out = {}
    for line in run.stdout.splitlines():
        name, *vals = line.split()
        if name == "status" and len(vals) == 2:
            out.setdefault("counts", {})[int(vals[0])] = int(vals[1])
        elif vals and all("0x" in v or v in ("inf", "-inf", "nan", "-nan") for v in vals):
            out[name] = np.array([float.fromhex(v) if "0x" in v else float(v) for v in vals], np.float64)
        else:
            out[name] = tuple(int(v) for v in vals)
    return run, out


def write_raw(path, M1, D1, M2, D2, R, T, W, H):
    """the `raw` mode's input: 58 doubles as hex floats, then W and H"""
    vals = np.concatenate([np.asarray(a, np.float64).reshape(-1) for a in (M1, D1, M2, D2, R, T)])
    assert vals.size == 58
    open(path, "w").write(" ".join(float(v).hex() for v in vals) + " %d %d\n" % (W, H))
