"""CPU-side checks of the Anderson-accelerated closed-loop simulation
(Solver.simulate_batch(accel=m), raocp_cp_batch_mpc_aa, k_mpc_step_aa).

* csrc/raocp_aa_ops.h aa_count, the one definition of what a log record adds to the four counters
  of a step, through tests/accel/aa_count_main.cpp: a stand-alone program built with the host
  compiler and -fsanitize=address,undefined that reduces a log as the kernel does; its counts
  against a NumPy count of the same records (integers: exact).
* the Python side: BatchSimulation without accel_counts, the option normaliser shared by
  chock_batch and simulate_batch, and simulate_batch refusing bad options before any native call.
* the header, the binding and the kernel_info switch declare the entry point and op 20.
"""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import raocp.core as core
from raocp.core import _native
from raocp.core.solver import BatchSimulation, normalise_accel
from helpers import problem_from_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# every (code, prop) the log format allows (include/raocp_hip.h raocp_cp_batch_aa_log), each a
# different number of times so that no two counters can be mistaken for one another
COMBOS = [((0, 0), 7),   # a plain iteration
          ((1, 1), 5),   # a proposal made
          ((2, 0), 3),   # a trial accepted, nothing followed
          ((2, 1), 11),  # a trial accepted that went on to propose
          ((2, 2), 2),   # a trial accepted whose next solve was refused
          ((3, 0), 13),  # a trial rejected
          ((4, 2), 4)]   # a solve refused


def numpy_counts(log):
    """The four counters of a (rows, 12) log: proposals made, trials accepted, trials rejected,
    solves refused."""
    log = np.asarray(log).reshape(-1, 12)
    return np.array([np.count_nonzero(log[:, 2] == 1), np.count_nonzero(log[:, 0] == 2),
                     np.count_nonzero(log[:, 0] == 3), np.count_nonzero(log[:, 2] == 2)], dtype=np.int64)


def _hand_written_log(repeat, seed):
    rng = np.random.default_rng(seed)
    recs = []
    for (code, prop), n in COMBOS:
        for _ in range(n * repeat):
            r = np.zeros(12)
            r[0], r[1], r[2], r[3] = code, rng.integers(0, 6), prop, rng.random()
            r[4:] = rng.standard_normal(8)   # gamma: nothing a counter may look at
            recs.append(r)
    log = np.array(recs)
    return log[rng.permutation(len(log))]


@pytest.fixture(scope="module")
def count_exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("mpc_accel") / "aa_count")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "raocp-toolbox_amd", "csrc"),
                    os.path.join(ROOT, "tests", "accel", "aa_count_main.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True, timeout=300)
    return exe


def _run(exe, log, path):
    np.savetxt(path, log, fmt="%.17g")
    p = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    lines = p.stdout.strip().split("\n")
    assert lines[1] == f"records {len(log)}"
    return np.array([int(v) for v in lines[0].split()[1:]], dtype=np.int64)


# 1: fewer records than lanes; 12: 540 records, every lane takes two or three
@pytest.mark.parametrize("repeat", [1, 12])
def test_header_counts_every_combination(count_exe, tmp_path, repeat):
    log = _hand_written_log(repeat, seed=repeat)
    assert {(int(r[0]), int(r[2])) for r in log} == {c for c, _ in COMBOS}
    got = _run(count_exe, log, tmp_path / "log.txt")
    want = numpy_counts(log)
    n = {c: k * repeat for c, k in COMBOS}
    # the NumPy count against the multiplicities the log was written with
    assert want.tolist() == [n[(1, 1)] + n[(2, 1)], n[(2, 0)] + n[(2, 1)] + n[(2, 2)], n[(3, 0)], n[(2, 2)] + n[(4, 2)]]
    assert np.array_equal(got, want), (got, want)


def test_header_counts_one_record_each_and_none(count_exe, tmp_path):
    for (code, prop), _ in COMBOS:
        rec = np.zeros((1, 12))
        rec[0, 0], rec[0, 2] = code, prop
        assert np.array_equal(_run(count_exe, rec, tmp_path / "one.txt"), numpy_counts(rec)), (code, prop)
    assert _run(count_exe, np.zeros((0, 12)), tmp_path / "none.txt").tolist() == [0, 0, 0, 0]


def test_batch_simulation_without_accel_counts():
    a = [np.zeros(1)] * 7
    r = BatchSimulation(*a)
    assert r.accel_counts is None and r.scenarios is a[6]
    c = np.zeros((1, 1, 4), dtype=np.int64)
    assert BatchSimulation(*a, accel_counts=c).accel_counts is c
    assert BatchSimulation(*a, c).accel_counts is c


def test_normalise_accel():
    assert normalise_accel(0) is None and normalise_accel(0, 0, -1.0, -1.0) is None   # off: nothing is looked at
    assert normalise_accel(5) == (5, 1, 1e-10, 1.0)
    out = normalise_accel(np.int64(8), np.int32(3), 0, 0)
    assert out == (8, 3, 0.0, 0.0) and [type(v) for v in out] == [int, int, float, float]
    assert normalise_accel(1, 2, 1e-6, 1e300) == (1, 2, 1e-6, 1e300)
    for bad in (9, -1, 2.5, 100, "5", 9.0):
        with pytest.raises(ValueError, match="accel must be 0 or in 1 .. 8"):
            normalise_accel(bad)
    for kw in (dict(accel_every=0), dict(accel_every=-3), dict(accel_reg=-1e-12), dict(accel_safeguard=-1.0),
               dict(accel_reg=float("nan")), dict(accel_safeguard=float("nan"))):
        with pytest.raises(ValueError, match="accel_every must be >= 1, accel_reg and accel_safeguard >= 0"):
            normalise_accel(5, **kw)


class _NoNative:
    """Stands where the solver's native context is: any use of it is a failure."""

    def __getattr__(self, name):
        raise AssertionError(f"native call {name} before the options were checked")


def test_simulate_batch_checks_the_options_before_any_native_call(golden, monkeypatch):
    _, _, prob = problem_from_golden(golden("main_trace"), "main")
    monkeypatch.setattr(core.Cache, "__init__", lambda self, *a, **k: None)
    monkeypatch.setattr(core.Cache, "native", _NoNative(), raising=False)
    monkeypatch.setattr(core.Operator, "__init__", lambda self, *a, **k: None)
    s = core.Solver(problem_spec=prob)
    X = np.zeros((2, 3))
    scen = np.zeros((2, 2), dtype=np.int64)
    for kw in (dict(accel=9), dict(accel=-1), dict(accel=2.5), dict(accel=5, accel_every=0),
               dict(accel=5, accel_reg=-1.0), dict(accel=5, accel_safeguard=-1.0)):
        with pytest.raises(ValueError, match="accel"):
            s.simulate_batch(X, 2, scenarios=scen, step_size=0.1, **kw)
        with pytest.raises(ValueError, match="accel"):
            s.chock_batch(X, step_size=0.1, **kw)
    assert s.batch_simulation is None and s.batch_accel_log == []
    # valid options do reach the native layer
    with pytest.raises(AssertionError, match="native call"):
        s.simulate_batch(X, 2, scenarios=scen, step_size=0.1, accel=5)


def test_header_binding_and_switch_declare_the_entry_point():
    text = open(os.path.join(ROOT, "include", "raocp_hip.h")).read()
    m = re.search(r"\bint\s+raocp_cp_batch_mpc_aa\s*\(([^;]*)\);", text)
    assert m and "int* aa_counts" in m.group(1) and "accel_safeguard" in m.group(1)
    assert "raocp_cp_batch_mpc_aa" in _native.EXPORTED_SYMBOLS
    assert "op 20" in text
    capi = open(os.path.join(ROOT, "raocp-toolbox_amd", "csrc", "raocp_capi.hip")).read()
    assert re.search(r"case 20:.*\n.*mpc_step_aa_name\(\)", capi)
