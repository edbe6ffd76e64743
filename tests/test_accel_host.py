"""CPU: the host-compilable parts of the Anderson-accelerated batch kernel.

* csrc/raocp_aa_ops.h (the regularised Cholesky solve k_cpa calls) and csrc/raocp_cpa_layout.h (the
  acceleration's slab) through tests/accel/aa_host_main.cpp, a stand-alone program built with the
  host compiler and -fsanitize=address,undefined; the program states its bounds.
* tests/accel_ref.py: its own solve against numpy.linalg.solve, the free model's decisions on
  main.py's problem, and replay of the free model's log reproducing the free run bit for bit.
* The inputs of tests/test_gpu_accel_grid.py and of the grid tests of tests/test_gpu_mpc_accel.py: the
  free model alone meets every coverage condition of tests/accel_cases.py on every case of the grid,
  and with accel_reg = inf it refuses every solve, where the closed form says.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import accel_cases as ac
import accel_ref
import branch_cases as bc
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


def test_header_refuses_an_infinite_regularisation(host_out):
    assert [l for l in host_out if l.startswith("reginf")] == ["reginf j1=0 j4=0 j8=0 zero1=0 zero4=0 zero8=0 ok"]


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


@pytest.mark.parametrize("tree", ac.TREES)
def test_free_model_meets_the_coverage_conditions_on_the_grid(tree):
    """What tests/test_gpu_accel_grid.py asserts on the device's log, on the reference alone: every
    case of the grid fills its ring, overwrites every slot after the wrap, pushes off the cadence and
    mixes rejections with proposals as accel_cases.coverage_violations states."""
    r, prob, op, alpha = bc.problem(tree)
    X = ac.states(tree)
    for opt in [o for t, o in ac.CASES if t == tree]:
        m, every, reg, sg = ac.OPTS[opt]
        for b in range(3):
            free = accel_ref.run(op, X[b], alpha, ac.K, 0.0, m=m, every=every, reg=reg, safeguard=sg)
            codes = np.bincount(free.log[:, 0].astype(int), minlength=5).tolist()
            assert free.log.shape == (ac.K + 1, 12)
            assert ac.coverage_violations(free.log, opt) == [], (tree, opt, b, codes)
            assert ac.gamma_violations(free.log) == [], (tree, opt, b)


# (tree, m, every) of the grid of tests/test_gpu_mpc_accel.py: step 0 of every instance is this cold solve
@pytest.mark.parametrize("tree,m,every", [("main", 1, 1), ("main", 8, 1), ("main", 3, 3), ("s5x3", 8, 1), ("m7x32", 8, 1)])
def test_free_model_fills_the_ring_in_30_iterations(tree, m, every):
    r, prob, op, alpha = bc.problem(tree)
    for x in ac.states(tree):
        free = accel_ref.run(op, x, alpha, 30, 0.0, m=m, every=every)
        assert free.log[:, 1].max() == m and np.count_nonzero(free.log[:, 2] == 1) >= 5, free.log[:, :3].astype(int).tolist()


@pytest.mark.parametrize("every", [1, 3])
@pytest.mark.parametrize("m", [1, 5, 8])
def test_model_refuses_every_solve_with_an_infinite_regularisation(m, every, recwarn):
    """reg = inf: every system is refused (no NumPy warning: the shift goes to the diagonal only),
    the history is cleared, and the refusals are where accel_cases.refusals_of counts them."""
    r, prob, op, alpha = bc.problem("main")
    x0 = np.asarray(r["x0"], dtype=float).reshape(-1)
    for K in (30, 31):
        ref = accel_ref.run(op, x0, alpha, K, 0.0, m=m, every=every, reg=float("inf"))
        code, j, prop = (ref.log[:, q].astype(int) for q in range(3))
        hit = np.flatnonzero(code == 4)
        assert set(code) == {0, 4} and np.array_equal(code == 4, prop == 2) and not ref.log[:, 4:].any()
        assert hit.size == ac.refusals_of(K + 1, every) and np.all(j[hit + 1] == 0) and code[-1] == 0
        assert np.array_equal(hit, np.arange(1, K, 2) if every == 1 else np.arange(every - 1, K, every))
        _, perr, _, pz, _, _ = op.chock(x0, K, 0.0, alpha=alpha)
        assert np.array_equal(ref.err, perr) and np.array_equal(ref.z, pz)
    assert len(recwarn) == 0
