"""The tier planner of the tiered dynamics sweep on the host (csrc/raocp_tierplan.h, no HIP
dependency): tests/tierplan/plan_host_main.cpp, a stand-alone program built with the host
compiler and -fsanitize=address,undefined, builds regular trees in memory (one class per stage,
one kind and one pair per child slot), plans them for 256 CUs and compares the whole result (the
top's cut, LDS bytes, widest stage, F-in-LDS and fold choices, and per tier its stage range,
widest level, LDS bytes of both kernels, F mode and fold) with expected values written into the
program: binary N = 12 at 20 / 8 (config 2) with fold allowed, fold disallowed and per-stage
forced; branching 4, N = 5 at 20 / 8; binary N = 3 at 3 / 2 (all of it lands in the top); binary
N = 4 at 64 / 32 (F per level); binary N = 4 at 96 / 48 (nothing fits: cut 0). Trees with more than
four children per node (5-ary, 8-ary, ragged, a root of 82) have no recorded plan: the program checks
that the top and the tiers tile the parent stages exactly once, or that the planner declines.

Where the expected numbers come from: the planning block of raocp_ctx_create as it stood before
the planner was split out (the commit before this file was added), lifted unchanged into a
throw-away host program with the same trees and 256 CUs, and its printed output copied here. They
are not derived from raocp_tierplan.h. The comparison is exact (integers and flags).
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tier_plans_match_recorded_plans(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "plan_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "raocp-toolbox_amd", "csrc"),
                    os.path.join(ROOT, "tests", "tierplan", "plan_host_main.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True, timeout=300)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(p.stdout)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "0 of 7 plans differ" in p.stdout
    # 5-ary, 8-ary, ragged (1 .. 12 and 1 .. 6 children) and wide-root stage profiles: every parent stage
    # in exactly one tier, or the planner declines (plan_host_main.cpp: covers)
    assert "0 of 6 wide profiles broken" in p.stdout and "BROKEN" not in p.stdout
