"""The composed maps of the regular-tree sweep on the host (csrc/raocp_drxfer.h, no HIP
dependency): tests/dr_xfer/xfer_host_main.cpp, a stand-alone program built with the host
compiler and -fsanitize=address,undefined, composes the root map of a binary tier with 4 levels
(nx = 20, nu = 8) from random stage matrices of spectral norm <= 1, applies its packed image in
the kernel's summation order and compares with the level recursion in long double. Bound: 1e-12
relative (the project's rounding-level tolerance: 720-term dot products of O(1) entries in
fp64 land at a few 1e-16 sqrt(720)). The program prints the error of every trial.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_composed_root_map_matches_level_recursion(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "xfer_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "raocp-toolbox_amd", "csrc"),
                    os.path.join(ROOT, "tests", "dr_xfer", "xfer_host_main.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True, timeout=300)
    p = subprocess.run([exe, "1e-12"], capture_output=True, text=True, timeout=120)
    print(p.stdout)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "worst rel err" in p.stdout
