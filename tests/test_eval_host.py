"""CPU: the evaluation of a solve on the host.

* tests/eval_ref.py's AVaR (greedy sorted fill) against scipy.optimize.linprog on the ambiguity
  set {alpha mu <= p, mu >= 0, 1'mu = 1}: this pins the reference the GPU tests compare against,
  independently of any code under test. Bound 1e-12 (two exact algorithms on O(1) data).
* csrc/raocp_eval_ops.h through tests/eval/avar_host_main.cpp, a stand-alone program built with
  the host compiler and -fsanitize=address,undefined: its AVaR (the Rockafellar-Uryasev minimum,
  the routine the kernels call) against the same LP on the same cases, and the launch plan of the
  backward sweep for a binary tree of N = 9 and a ternary one of N = 5.
* eval_ref.evaluate on OracleProblem.chock solutions reproduces recorded figures (1e-9 relative).
"""
import os
import shutil
import subprocess

import numpy as np
import pytest
from scipy.optimize import linprog

import eval_ref
from oracle.raocp_oracle import OracleProblem
from raocp.problems import build_problem, recipe_general_small, recipe_main

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALPHAS = (0.0, 0.05, 0.1, 0.5, 0.7, 0.95, 0.99, 1.0)
TOL = 1e-12


def _lp(Z, p, alpha):
    """max mu'Z over {alpha mu <= p, mu >= 0, 1'mu = 1} by the LP solver. alpha mu_k <= p_k is
    handed over as the variable's upper bound p_k / alpha: as a constraint row, HiGHS drops a right
    side of 1e-12 as zero, and the LP's own value is then off by p_k |Z_k| (5e-12 measured here,
    against 9e-16 with bounds)."""
    c = len(Z)
    bounds = [(0, None if alpha <= 0 else p[k] / alpha) for k in range(c)]
    res = linprog(-np.asarray(Z), A_eq=np.ones((1, c)), b_eq=[1.0], bounds=bounds, method="highs")
    assert res.status == 0, res.message
    return -res.fun


def _cases():
    """Seeded cases: c = 1 .. 6 and 17, 65, 82, every alpha of ALPHAS, random outcomes, ties (outcomes drawn from
    three values, all equal) and probabilities as small as 1e-12."""
    rng = np.random.default_rng(20240)
    out = []
    for c in range(1, 7):
        for alpha in ALPHAS:
            for kind in ("random", "ties", "equal", "tiny_p"):
                Z = rng.standard_normal(c) * 3.0
                if kind == "ties":
                    Z = rng.choice(np.array([-1.5, 0.25, 2.0]), size=c)
                elif kind == "equal":
                    Z = np.full(c, float(rng.standard_normal()))
                p = rng.random(c) + 0.05
                if kind == "tiny_p" and c > 1:
                    p[rng.integers(c)] = 1e-12
                p /= p.sum()
                out.append((Z, p, alpha))
    # wide families (17, 65 and 82 outcomes, the child counts of branch_cases.WIDE), drawn after the
    # cases above so that those keep their values: the same kinds, and a child of probability zero
    for c in (17, 65, 82):
        for alpha in ALPHAS:
            for kind in ("random", "ties", "equal", "tiny_p", "zero_p"):
                Z = rng.standard_normal(c) * 3.0
                if kind == "ties":
                    Z = rng.choice(np.array([-1.5, 0.25, 2.0]), size=c)
                elif kind == "equal":
                    Z = np.full(c, float(rng.standard_normal()))
                p = rng.random(c) + 0.05
                if kind == "tiny_p":
                    p[rng.integers(c)] = 1e-12
                elif kind == "zero_p":
                    p[int(np.argmax(Z))] = 0.0  # the worst outcome cannot happen
                    p[rng.integers(c)] = 0.0
                p /= p.sum()
                out.append((Z, p, alpha))
    return out


CASES = _cases()


def test_reference_avar_equals_the_lp():
    worst = 0.0
    for Z, p, alpha in CASES:
        worst = max(worst, abs(eval_ref.avar(Z, p, alpha) - _lp(Z, p, alpha)))
    print(f"greedy fill vs linprog over {len(CASES)} cases: {worst:.2e}")
    assert worst <= TOL


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("eval") / "avar_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "raocp-toolbox_amd", "csrc"),
                    os.path.join(ROOT, "tests", "eval", "avar_host_main.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True, timeout=300)
    return exe


def _run(exe, lines):
    p = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    return p.stdout.split("\n")


def test_header_avar_equals_the_lp(host_exe):
    lines = ["A %d %r %s %s" % (len(Z), alpha, " ".join(repr(float(v)) for v in Z), " ".join(repr(float(v)) for v in p))
             for Z, p, alpha in CASES]
    got = [float(s.split()[1]) for s in _run(host_exe, lines) if s.startswith("A ")]
    assert len(got) == len(CASES)
    worst = max(abs(g - _lp(Z, p, alpha)) for g, (Z, p, alpha) in zip(got, CASES))
    print(f"avar_ru vs linprog over {len(CASES)} cases: {worst:.2e}")
    assert worst <= TOL
    # the special cases by name: alpha = 0 the maximum, alpha = 1 the expectation, one child
    for g, (Z, p, alpha) in zip(got, CASES):
        if alpha == 0.0:
            assert g == Z.max()
        if alpha == 1.0:
            assert abs(g - p @ Z) <= TOL
        if len(Z) == 1:
            assert g == Z[0]


def test_header_avar_with_float_probabilities(host_exe):
    """The form an fp32 context runs: probabilities held as float, arithmetic in double, against
    the LP on the unrounded probabilities. The minimand t + sum_k p_k max(Z_k - t, 0) / alpha moves
    by at most sum_k |dp_k| (max Z - min Z) / alpha when p moves by dp, |dp_k| <= 2^-24 p_k <= 2^-24."""
    lines = ["F %d %r %s %s" % (len(Z), alpha, " ".join(repr(float(v)) for v in Z), " ".join(repr(float(v)) for v in p))
             for Z, p, alpha in CASES]
    got = [float(s.split()[1]) for s in _run(host_exe, lines) if s.startswith("A ")]
    assert len(got) == len(CASES)
    for g, (Z, p, alpha) in zip(got, CASES):
        bound = TOL if alpha == 0.0 else 2.0 ** -24 * len(Z) * (Z.max() - Z.min()) / alpha + TOL
        assert abs(g - _lp(Z, p, alpha)) <= bound, (Z, p, alpha, g)


def _plan(host_exe, stage_ptr):
    out = _run(host_exe, ["P %d %s" % (len(stage_ptr), " ".join(map(str, stage_ptr)))])
    n = int(out[0].split()[1])
    return [tuple(int(v) for v in s.split()[1:]) for s in out[1:1 + n]]


@pytest.mark.parametrize("C,N,expect", [
    # binary N = 9 (1,023 nodes): stages 8 (256 parents) and 7 (128) alone, 6 .. 0 in the last launch
    (2, 9, [(8, 8, 4, 0), (7, 7, 2, 0), (6, 0, 1, 1)]),
    # ternary N = 5 (364 nodes): stage 4 (81 parents) alone, 3 .. 0 (27, 9, 3, 1) in the last launch
    (3, 5, [(4, 4, 2, 0), (3, 0, 1, 1)]),
])
def test_sweep_plan_covers_every_parent_stage_once(host_exe, C, N, expect):
    width = [C ** t for t in range(N + 1)]
    stage_ptr = [int(v) for v in np.concatenate([[0], np.cumsum(width)])]
    plan = _plan(host_exe, stage_ptr)
    assert plan == expect
    stages = [t for hi, lo, _, _ in plan for t in range(hi, lo - 1, -1)]
    assert stages == list(range(N - 1, -1, -1))  # every parent stage once, deepest first
    for hi, lo, blocks, last in plan[:-1]:
        assert hi == lo and not last and blocks == -(-width[hi] // 64) and width[hi] > 64
    assert plan[-1][3] == 1 and plan[-1][2] == 1 and all(width[t] <= 64 for t in range(plan[-1][0] + 1))


def _relerr(got, ref):
    return abs(got - ref) / abs(ref)


def test_reference_on_oracle_solutions_main():
    """main.py's problem at its own tol = 1e-3 (937 rows): the cost and s_0 differ by 0.8 %."""
    r = recipe_main()
    orc = OracleProblem(build_problem(r)[1])
    alpha = float(np.load(os.path.join(ROOT, "tests", "golden", "main_trace.npz"))["main/cp_alpha"])
    st, err, _, z, _, _ = orc.chock(r["x0"], 2000, 1e-3, alpha=alpha)
    assert st == 0 and err.shape[0] == 937
    cost, s0, box, dyn, V = eval_ref.evaluate(orc, z, r["x0"])
    print(f"main: cost {cost!r} s0 {s0!r} box {box!r} dyn {dyn!r}")
    assert _relerr(cost, 1.2522228374539) <= 1e-9
    assert _relerr(s0, 1.2423913282094) <= 1e-9
    assert dyn <= 1e-14 and box == 0.0


def test_reference_on_oracle_solutions_g53():
    """g53 after 3000 iterations at tol 0: converged, so the cost and s_0 agree."""
    r = recipe_general_small("g53")
    orc = OracleProblem(build_problem(r)[1])
    _, _, _, z, _, _ = orc.chock(r["x0"], 2999, 0.0)
    cost, s0, box, dyn, V = eval_ref.evaluate(orc, z, r["x0"])
    print(f"g53: cost {cost!r} s0 {s0!r} box {box!r} dyn {dyn!r}")
    assert _relerr(cost, 4.448456039332924) <= 1e-9
    assert _relerr(s0, 4.448456039332891) <= 1e-9
    assert abs(cost - s0) <= 1e-12 * abs(cost)
