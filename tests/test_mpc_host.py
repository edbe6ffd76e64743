"""CPU-side checks of the closed-loop batch simulation (Solver.simulate_batch): the scenario
normaliser, the seeded sampler and the C-ABI declaration."""
import os
import re

import numpy as np
import pytest

from raocp.core.solver import normalise_scenarios, sample_scenarios
from raocp.core import _native
from helpers import problem_from_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_normalise_scenarios_pass_through():
    a = np.array([[0, 1, 2], [2, 2, 0]], dtype=np.int64)
    out = normalise_scenarios(a, 2, 3, 3)
    assert out.shape == (2, 3) and out.dtype == np.int32 and out.flags["C_CONTIGUOUS"]
    assert np.array_equal(out, a)
    assert np.array_equal(normalise_scenarios([[0, 1, 2], [2, 2, 0]], 2, 3, 3), a)
    assert normalise_scenarios(a.T.copy().T, 2, 3, 3).flags["C_CONTIGUOUS"]
    assert normalise_scenarios(np.zeros((4, 0), dtype=np.int32), 4, 0, 3).shape == (4, 0)


@pytest.mark.parametrize("bad", [
    np.zeros((2, 4), dtype=np.int32),          # (B, T + 1)
    np.zeros((3, 3), dtype=np.int32),          # (B + 1, T)
    np.zeros(6, dtype=np.int32),               # flat
    np.zeros((2, 3, 1), dtype=np.int32),
    np.zeros((2, 3)),                          # float dtype
    np.zeros((2, 3), dtype=bool),
    np.array([[0, 1, 3], [0, 0, 0]]),          # entry == n_children
    np.array([[0, 1, 2], [0, -1, 0]]),         # negative entry
])
def test_normalise_scenarios_rejects(bad):
    with pytest.raises(ValueError):
        normalise_scenarios(bad, 2, 3, 3)


def test_sampler_is_seeded_and_follows_the_root_probabilities(golden):
    _, tree, _ = problem_from_golden(golden("main_trace"), "main")
    p = np.asarray(tree.conditional_probabilities_of_children(0), dtype=float)
    assert np.allclose(p, (0.1, 0.6, 0.3), atol=1e-12)
    a = sample_scenarios(p, 200, 100, seed=3)
    assert a.shape == (200, 100) and a.dtype == np.int32
    assert np.array_equal(a, sample_scenarios(p, 200, 100, seed=3))
    assert not np.array_equal(a, sample_scenarios(p, 200, 100, seed=4))
    freq = np.bincount(a.reshape(-1), minlength=3) / a.size    # 20,000 draws
    print("frequencies", freq)
    assert freq.shape == (3,) and np.all(np.abs(freq - (0.1, 0.6, 0.3)) <= 0.02)
    # the draws pass the normaliser unchanged
    assert np.array_equal(normalise_scenarios(a, 200, 100, 3), a)


def test_header_and_binding_declare_the_entry_point():
    text = open(os.path.join(ROOT, "include", "raocp_hip.h")).read()
    assert re.search(r"\bint\s+raocp_cp_batch_mpc\s*\(\s*raocp_ctx\s*\*", text)
    assert "raocp_cp_batch_mpc" in _native.EXPORTED_SYMBOLS
