"""CPU: the host-compilable parts of the Anderson-accelerated batch kernel.

* csrc/raocp_aa_ops.h (the regularised Cholesky solve k_cpa calls) and csrc/raocp_cpa_layout.h (the
  acceleration's slab) through tests/accel/aa_host_main.cpp, a stand-alone program built with the
  host compiler and -fsanitize=address,undefined; the program states its bounds.
* tests/accel_ref.py: its own solve against numpy.linalg.solve, the free model's decisions on
  main.py's problem, and replay of the free model's log reproducing the free run bit for bit.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import accel_ref
from oracle.raocp_oracle import OracleProblem
from helpers import problem_from_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host_out(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("accel") / "aa_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "raocp-toolbox_amd", "csrc"),
                    os.path.join(ROOT, "tests", "accel", "aa_host_main.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True, timeout=300)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(p.stdout)
    assert p.returncode == 0, p.stdout + p.stderr
    return p.stdout.strip().split("\n")


def test_header_solve_against_long_double(host_out):
    lines = [l for l in host_out if l.startswith("solve")]
    assert len(lines) == 8 and all(l.endswith(" ok") for l in lines), lines


def test_header_refuses_a_bad_pivot(host_out):
    assert [l for l in host_out if l.startswith("refuse")] == ["refuse indefinite=0 zero=0 nan=0 j0=0 j9=0 identity=1 ok"]


def test_layout_aligned_and_disjoint(host_out):
    line = [l for l in host_out if l.startswith("layout")]
    # main.py at m = 5: (2 * 5 + 3) vectors of 1,236 doubles, G and the state block: 128 KB
    assert line == ["layout main m=5 stride 16160 doubles ok"], line


def test_model_solve():
    rng = np.random.default_rng(3)
    for j in range(1, 9):
        dR = list(rng.standard_normal((j, 3 * j + 5)))
        r = rng.standard_normal(3 * j + 5)
        Gb, b = accel_ref.aa_system(dR, r, 1e-10)
        g = accel_ref.aa_solve(Gb, b)
        assert np.linalg.norm(g - np.linalg.solve(Gb, b)) <= 1e-12 * np.linalg.norm(g)
    assert accel_ref.aa_solve(np.array([[1.0, 2.0], [2.0, 1.0]]), np.ones(2)) is None
    assert accel_ref.aa_solve(np.zeros((2, 2)), np.ones(2)) is None


def test_model_free_and_replay(golden):
    z = golden("main_trace")
    r, tree, prob = problem_from_golden(z, "main")
    orc = OracleProblem(prob)
    x0 = np.asarray(r["x0"], dtype=float).reshape(-1)
    alpha = float(z["main/cp_alpha"])
    free = accel_ref.run(orc, x0, alpha, 40, 0.0, m=5)
    codes = free.log[:, 0].astype(int)
    assert free.err.shape == (41, 3) and codes[0] == 0 and codes[1] == 1 and set(codes[2:]) <= {2, 3}
    for k, lhs, rhs, code in free.trials:
        assert code == (2 if lhs <= rhs else 3)
    again = accel_ref.run(orc, x0, alpha, 40, 0.0, m=5, log=free.log)
    assert np.array_equal(again.err, free.err) and np.array_equal(again.z, free.z) and np.array_equal(again.log, free.log)
    # every trial rejected: the rows that are no trials are the plain solve's, bit for bit
    rej = accel_ref.run(orc, x0, alpha, 30, 0.0, m=5, safeguard=0.0)
    keep = rej.log[:, 0] != 3
    _, perr, _, _, _, _ = orc.chock(x0, 30, 0.0, alpha=alpha)
    assert np.array_equal(rej.err[keep], perr[:int(keep.sum())])
