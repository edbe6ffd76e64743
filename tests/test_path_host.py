"""Which kernels a context runs, as a host function (csrc/raocp_path.h, no HIP dependency):
tests/path/path_host_main.cpp, a stand-alone program built with the host compiler and
-fsanitize=address,undefined, run directly with nothing preloaded and no GPU.

(a) Named capability sets (config 2 by default and under RAOCP_DRC=0 / RAOCP_CP6=0, configs 4 and
5, the tier sweeps with and without the split form, the scalar CP kernels, dyn2, nothing), unsharded
and as a shard, with the dynamics path, CP path and fused flag written into the program.

(b) All 2^11 capability sets times {unsharded, sharded} = 4,096 combinations against two plain if
cascades in the program, one for the dynamics and one for the CP kernels.

Where the expected values come from: the precedence chains the library spelled out at each use
site before resolve_paths existed (the commit before this file was added): launch_dynamics with
DynOp::run, and enqueue_cp_iteration with launch_cp3 and launch_cpd / launch_cpp, their conditions
copied in order. They are not derived from raocp_path.h. The comparison is exact.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_resolved_paths_match_the_recorded_chains(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "path_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "raocp-toolbox_amd", "csrc"),
                    os.path.join(ROOT, "tests", "path", "path_host_main.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True, timeout=300)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(p.stdout)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "0 of 13 named cases differ" in p.stdout
    assert "0 mismatches over 4096 combinations" in p.stdout
