"""The allocation list and the create-failure epilogue of the C ABI layer (rt-depth-map_amd/csrc/rtdm_host.h), through the
stand-alone program tests/alloc_host.cpp: built with hipcc (host code only, linked against the HIP runtime) into a temporary
directory.  Without a HIP device every request of the program fails, which is the path a create function takes when an
allocation fails half way; with a device the program makes one absurd request fail itself."""
import os
import subprocess

from conftest import ROOT


def test_allocation_list_keeps_the_first_error_and_releases_what_it_holds(tmp_path):
    exe = str(tmp_path / "alloc_host")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "rt-depth-map_amd", "csrc"),
                           os.path.join(ROOT, "tests", "alloc_host.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.startswith("ok: 0 failed checks"), run.stdout + run.stderr
