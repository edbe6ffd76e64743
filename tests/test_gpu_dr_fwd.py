"""GPU parity of the forward sweep by superposition in the regular-tree sweep (raocp_dynr.hip
tier_body with raocp_drxfer.h xf_compose): a tier below the top runs its four forward levels
from a zero root x row while it waits for that row, and adds the composed map's product with
the row once it has landed. RAOCP_DR_FWD=0 switches off this path alone, RAOCP_DR_XFER=0 every
composed map. The rows are the same quantities to rounding, so the settings agree at the
project's rounding-level tolerance, 1e-12, for the projection alone (k_dr, which
project_on_dynamics launches under either RAOCP_DRC setting; the setting only selects the context
the plan is built for) and over 30 CP iterations (k_drc; a graph batch boundary at 24 inside);
against the oracle the bounds are those of test_gpu_drc.py (1e-8 per trace entry, 1e-10 on the iterate). Every output has one
owner lane and a fixed summation order: the projection of the same input twice is bit-identical.

Cases: bin8 and markov8 (511 nodes, two tiers: the smallest shape with a deepest tier below a
top), c2 boxed and unboxed (8,191 nodes, three tiers: the only shape with a middle tier; k_drc
has an instantiation for each, and the unboxed one keeps the level path: op 16 is "" there and
the three settings run the same code), bin4 (31 nodes, the top alone: no forward map).
raocp_kernel_info op 16 names the active forward maps; op 15 is unchanged.
"""
import numpy as np
import pytest

import raocp.core as core
from raocp.problems import build_problem
from helpers import rel_err, trace_rel_err
from test_gpu_drc import _case, _close, _run, _with_env

pytestmark = pytest.mark.gpu

CASES = ["bin8", "markov8", "c2", "bin4"]
# (the unboxed k_drc holds no forward-map step, so a context that runs it keeps the level path)
FWD = {"bin8": "deep_fwd@1", "markov8": "deep_fwd@1", "c2": "mid_fwd@1 deep_fwd@2", "c2-nobox": "", "bin4": ""}
BACK = {"bin8": "", "markov8": "", "c2": "mid_back_root@1", "c2-nobox": "mid_back_root@1", "bin4": ""}
SWITCHES = ({}, {"RAOCP_DR_FWD": "0"}, {"RAOCP_DR_XFER": "0"})

_problems = {}


def _problem(case):
    if case not in _problems:
        r, cuts = _case(case)
        _problems[case] = (r, cuts, build_problem(r)[1])
    return _problems[case]


def _trio(case, extra=None):
    """(recipe, problem, caches: default, RAOCP_DR_FWD=0, RAOCP_DR_XFER=0), all under `extra`"""
    r, cuts, prob = _problem(case)
    env = dict(extra or {})
    if cuts is not None:
        env["RAOCP_DR_CUTS"] = cuts
    return r, prob, [_with_env(dict(env, **sw), lambda: core.Cache(prob)) for sw in SWITCHES]


def _check_ops(case, caches):
    on, nofwd, off = caches
    assert on.native.kernel_info(16) == FWD[case]
    assert nofwd.native.kernel_info(16) == off.native.kernel_info(16) == ""
    assert on.native.kernel_info(15) == nofwd.native.kernel_info(15) == BACK[case]
    assert off.native.kernel_info(15) == ""


def _project(cache, r, zz):
    cache.cache_initial_state(r["x0"])
    cache.native.set_primal(zz)
    cache.native.project_on_dynamics()
    return cache.native.get_primal()


@pytest.mark.parametrize("drc", ["1", "0"])
@pytest.mark.parametrize("case", CASES)
def test_fwd_projection_matches_level_paths(case, drc):
    r, prob, caches = _trio(case, {"RAOCP_DRC": drc})
    _check_ops(case, caches)
    for c in caches:
        assert c.native.kernel_info(9) == "k_dr<20, 8> x1"
        assert c.native.kernel_info(11) == ("k_drc<20, 8, 2>" if drc == "1" else "")
    zz = np.random.default_rng(11).standard_normal(caches[0].primal_size)
    z1 = _project(caches[0], r, zz)
    again = _project(caches[0], r, zz)
    assert np.array_equal(z1, again), "the same input twice: not bit-identical"
    for name, c in (("RAOCP_DR_FWD=0", caches[1]), ("RAOCP_DR_XFER=0", caches[2])):
        e = rel_err(z1, _project(c, r, zz))
        print(f"{case} RAOCP_DRC={drc}: projection, forward map against {name}: rel err {e:.3e}")
        assert e <= 1e-12


@pytest.mark.parametrize("case", CASES + ["c2-nobox"])
def test_fwd_cp_loop_matches_level_paths_and_oracle(case):
    from oracle.raocp_oracle import OracleProblem
    r, prob, caches = _trio(case)
    _check_ops(case, caches)
    for c in caches:
        assert c.native.kernel_info(11) == "k_drc<20, 8, 2>"
    alpha = 0.999 / caches[0].native.step_size()
    K = 30
    a = _run(caches[0], r["x0"], K, alpha)
    assert a[0] == 1 and a[1].shape == (K + 1, 3)
    for name, c in (("RAOCP_DR_FWD=0", caches[1]), ("RAOCP_DR_XFER=0", caches[2])):
        b = _run(c, r["x0"], K, alpha)
        print(f"{case}: 30 iterations, forward map against {name}: trace {trace_rel_err(a[1], b[1]):.3e} / "
              f"{trace_rel_err(a[2], b[2]):.3e}, iterate {rel_err(a[3], b[3]):.3e} / {rel_err(a[4], b[4]):.3e}")
        _close(a, b)
    st_o, err_o, derr_o, z_o, e_o, _ = OracleProblem(prob).chock(r["x0"], K, 0.0, alpha=alpha)
    assert st_o == 1
    print(f"{case}: against the oracle: trace {trace_rel_err(a[1], err_o):.3e} / {trace_rel_err(a[2], derr_o):.3e}, "
          f"iterate {rel_err(a[3], z_o):.3e} / {rel_err(a[4], e_o):.3e}")
    assert trace_rel_err(a[1], err_o) <= 1e-8 and trace_rel_err(a[2], derr_o) <= 1e-8
    assert rel_err(a[3], z_o) <= 1e-10 and rel_err(a[4], e_o) <= 1e-10


def test_fwd_early_stop_inside_a_batch():
    """tol = a residual of the level path's loop (clear of rounding) at iteration 17, inside the
    first graph batch: the same status and iteration count with the forward map on and off."""
    r, prob, caches = _trio("c2")
    on, nofwd, off = caches
    alpha = 0.999 / on.native.step_size()
    _, err, _ = off.native.cp_run(r["x0"], 40, 0.0, alpha)
    tol = float(err[17].max()) * (1 + 1e-9)
    first = int(np.argmax(err.max(axis=1) <= tol))
    a = _run(on, r["x0"], 40, alpha, tol)
    for c in (nofwd, off):
        b = _run(c, r["x0"], 40, alpha, tol)
        assert a[0] == b[0] == 0 and a[1].shape == b[1].shape == (first + 1, 3)
        _close(a, b)


def test_fwd_info_op_five_level_tier():
    """Op 16 is empty on the N = 9 tree, whose plan has a 5-level tier (the level path of the
    other kernel build)."""
    from raocp.problems import recipe_synthetic
    r9 = recipe_synthetic(np.full((2, 2), .5), np.array([.5, .5]), 9, 9, 20, 8, seed=25)
    c9 = core.Cache(build_problem(r9)[1])
    assert c9.native.kernel_info(16) == "" and c9.native.kernel_info(15) == ""
