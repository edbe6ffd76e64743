"""CPU-side checks of the batched solve in either precision.

The slab map of k_cpb / k_mpc_step (csrc/raocp_cpb_layout.h, no HIP dependency) is exercised by
tests/cpb_layout/layout_host_main.cpp, a stand-alone program built with the host compiler and
-fsanitize=address,undefined, on the dimensions of the three problems the GPU tests use (main.py's
43-node tree, c1n5 and ops2x2; their sizes come from the oracle, which needs no GPU) and on the
largest sizes the kernel covers (nx 32, nu 16). For elements of 8 and 4 bytes: every offset times
the element size is a multiple of 16, the arrays are in order and do not overlap, the stride times
the element size is a multiple of 256, and the float slab is no larger in bytes than the double
one. The double map must also be the one the fp64 kernel had before the element size became a
parameter (lengths rounded to 2 doubles, stride to 32), recomputed here in Python."""
import os
import re
import shutil
import subprocess

import pytest

from oracle.raocp_oracle import OracleProblem
from helpers import problem_from_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBLEMS = [("main_trace", "main"), ("traj_small", "c1n5"), ("traj_small", "ops2x2")]


def _dims(golden):
    out = []
    for fixture, name in PROBLEMS:
        orc = OracleProblem(problem_from_golden(golden(fixture), name)[2])
        out.append((orc.P, orc.D, orc.n, orc.m, orc.nx, orc.nu))
    out.append((3 * 85 * 32, 11 * 85 * 32, 85, 21, 32, 16))   # the kernel's size limits, a 4-ary tree
    out.append((7, 5, 2, 1, 1, 1))                             # lengths that are no multiple of the 16-B unit
    return out


def _stride_of_fp64_map_before(P, D, n, m, nx, nu):
    at = 0
    for count in (P, P, P, D, D, D, D, n * nx, m * nu, n * (nx + nu), nx):
        at += (count + 1) // 2 * 2
    return (at + 31) // 32 * 32


def test_slab_maps_of_both_element_sizes(golden, tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "layout_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "raocp-toolbox_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpb_layout", "layout_host_main.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True, timeout=300)
    dims = _dims(golden)
    p = subprocess.run([exe] + [str(v) for d in dims for v in d], capture_output=True, text=True, timeout=120)
    print(p.stdout)
    assert p.returncode == 0, p.stdout + p.stderr
    m = re.search(r"^0 of (\d+) layout checks failed$", p.stdout, re.M)
    assert m and int(m.group(1)) == len(dims) * (2 * (2 + 3 * 11) + 1)
    strides = {(int(a.group(1)), int(a.group(2)), int(a.group(3))): int(a.group(4)) for a in re.finditer(
        r"^P (\d+) D (\d+) n \d+ m \d+ nx \d+ nu \d+ elt (\d): stride (\d+) elements", p.stdout, re.M)}
    for d in dims:
        assert strides[(d[0], d[1], 8)] == _stride_of_fp64_map_before(*d), d
        assert strides[(d[0], d[1], 4)] * 4 <= strides[(d[0], d[1], 8)] * 8, d


def test_both_precisions_are_instantiated_and_named():
    text = open(os.path.join(ROOT, "raocp-toolbox_amd", "csrc", "raocp_cpb.hip")).read()
    for inst in ("k_cpb<T, true>", "k_cpb<T, false>", "cpb_launch_t<float>", "cpb_launch_t<double>",
                 "k_mpc_step<float>", "k_mpc_step<double>"):
        assert inst in text, inst
    # the fp64 forms keep the names raocp_kernel_info reported before the kernels took a type
    for name in ('"k_cpb<true>"', '"k_cpb<false>"', '"k_mpc_step"', '"k_cpb<float, true>"', '"k_mpc_step<float>"'):
        assert name in text, name
    hdr = open(os.path.join(ROOT, "include", "raocp_hip.h")).read()
    assert "k_cpb<float" in hdr and "k_mpc_step<float>" in hdr
