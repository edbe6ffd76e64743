"""The forward map of the regular-tree sweep on the host (csrc/raocp_drxfer.h, no HIP
dependency): tests/dr_xfer/fwd_host_main.cpp, a stand-alone program built with the host
compiler and -fsanitize=address,undefined, composes the 720 x 20 map of a binary tier with 4
levels (nx = 20, nu = 8) from random [Abar_k | B_k] and K of spectral norm <= 1, runs the sweep
from x_0 = 0 in double in the kernel's order, adds the packed image's product with x_0 in the
kernel's order and compares every x and u row with the level recursion in long double. Bound:
1e-12 relative, the project's rounding-level tolerance (four levels of 28-long dots of O(1)
entries in fp64 land at a few 1e-16). The program prints the error of every trial.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_forward_map_matches_level_recursion(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "fwd_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "raocp-toolbox_amd", "csrc"),
                    os.path.join(ROOT, "tests", "dr_xfer", "fwd_host_main.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True, timeout=300)
    p = subprocess.run([exe, "1e-12"], capture_output=True, text=True, timeout=120)
    print(p.stdout)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "worst rel err" in p.stdout
