"""GPU parity of the composed maps in the regular-tree sweep (raocp_dynr.hip tier_body with
raocp_drxfer.h): a tier between the top and the deepest publishes its root's q row from one
composed product before its four backward levels. RAOCP_DR_XFER=0 keeps every row level by
level. The composed row and the level path's are the same quantity to rounding, so the two
settings agree at the project's rounding-level tolerance, 1e-12, for the projection alone
(k_dr and k_drc's plan) and over 30 CP iterations (a graph batch boundary at 24 inside);
against the oracle the bounds are those of test_gpu_drc.py (1e-8 per trace entry, 1e-10 on the
iterate).

Cases: bin8 and markov8 (511 nodes, two tiers: no tier between the top and the deepest, so no
composed map is active there and the two settings run the same code), c2 (8,191 nodes, three
tiers: the one shape with a middle tier). raocp_kernel_info op 15 names the active maps.
"""
import numpy as np
import pytest

import raocp.core as core
from raocp.problems import build_problem, recipe_synthetic
from helpers import rel_err, trace_rel_err
from test_gpu_drc import _case, _close, _run, _with_env

pytestmark = pytest.mark.gpu

CASES = ["bin8", "markov8", "c2"]
ACTIVE = {"bin8": "", "markov8": "", "c2": "mid_back_root@1"}


def _pair(case, extra=None):
    """(recipe, problem, default cache, RAOCP_DR_XFER=0 cache), both under `extra`"""
    r, cuts = _case(case)
    tree, prob = build_problem(r)
    env = dict(extra or {})
    if cuts is not None:
        env["RAOCP_DR_CUTS"] = cuts
    on = _with_env(env, lambda: core.Cache(prob))
    off = _with_env(dict(env, RAOCP_DR_XFER="0"), lambda: core.Cache(prob))
    return r, prob, on, off


def _project(cache, r, zz):
    cache.cache_initial_state(r["x0"])
    cache.native.set_primal(zz)
    cache.native.project_on_dynamics()
    return cache.native.get_primal()


@pytest.mark.parametrize("drc", ["1", "0"])
@pytest.mark.parametrize("case", CASES)
def test_xfer_projection_matches_level_path(case, drc):
    r, prob, on, off = _pair(case, {"RAOCP_DRC": drc})
    assert on.native.kernel_info(9) == off.native.kernel_info(9) == "k_dr<20, 8> x1"
    assert on.native.kernel_info(11) == off.native.kernel_info(11) == ("k_drc<20, 8, 2>" if drc == "1" else "")
    assert on.native.kernel_info(15) == ACTIVE[case] and off.native.kernel_info(15) == ""
    zz = np.random.default_rng(11).standard_normal(on.primal_size)
    z1 = _project(on, r, zz)
    z0 = _project(off, r, zz)
    e = rel_err(z1, z0)
    print(f"{case} RAOCP_DRC={drc}: projection, composed maps against the level path: rel err {e:.3e}")
    assert e <= 1e-12


@pytest.mark.parametrize("case", CASES)
def test_xfer_cp_loop_matches_level_path_and_oracle(case):
    from oracle.raocp_oracle import OracleProblem
    r, prob, on, off = _pair(case)
    assert on.native.kernel_info(11) == off.native.kernel_info(11) == "k_drc<20, 8, 2>"
    alpha = 0.999 / on.native.step_size()
    K = 30
    a = _run(on, r["x0"], K, alpha)
    b = _run(off, r["x0"], K, alpha)
    print(f"{case}: 30 iterations, composed maps against the level path: trace {trace_rel_err(a[1], b[1]):.3e} / "
          f"{trace_rel_err(a[2], b[2]):.3e}, iterate {rel_err(a[3], b[3]):.3e} / {rel_err(a[4], b[4]):.3e}")
    assert a[0] == 1 and a[1].shape == (K + 1, 3)
    _close(a, b)
    st_o, err_o, derr_o, z_o, e_o, _ = OracleProblem(prob).chock(r["x0"], K, 0.0, alpha=alpha)
    assert st_o == 1
    print(f"{case}: against the oracle: trace {trace_rel_err(a[1], err_o):.3e} / {trace_rel_err(a[2], derr_o):.3e}, "
          f"iterate {rel_err(a[3], z_o):.3e} / {rel_err(a[4], e_o):.3e}")
    assert trace_rel_err(a[1], err_o) <= 1e-8 and trace_rel_err(a[2], derr_o) <= 1e-8
    assert rel_err(a[3], z_o) <= 1e-10 and rel_err(a[4], e_o) <= 1e-10


def test_xfer_early_stop_inside_a_batch():
    """tol = a residual of the level path's loop (clear of rounding) at iteration 17, inside the
    first graph batch: the same status and iteration count with the switch on and off."""
    r, prob, on, off = _pair("c2")
    alpha = 0.999 / on.native.step_size()
    _, err, _ = off.native.cp_run(r["x0"], 40, 0.0, alpha)
    tol = float(err[17].max()) * (1 + 1e-9)
    first = int(np.argmax(err.max(axis=1) <= tol))
    a = _run(on, r["x0"], 40, alpha, tol)
    b = _run(off, r["x0"], 40, alpha, tol)
    assert a[0] == b[0] == 0 and a[1].shape == b[1].shape == (first + 1, 3)
    _close(a, b)


def test_xfer_info_op():
    """Op 15 names the active maps (tier index behind @), is empty under RAOCP_DR_XFER=0 and on
    the N = 9 tree, whose plan has a 5-level tier (the level path of the other kernel build)."""
    r, prob, on, off = _pair("c2")
    assert on.native.kernel_info(15) == "mid_back_root@1"
    assert off.native.kernel_info(15) == ""
    for op, want in ((9, "k_dr<20, 8> x1"), (10, "k_cp6<double, 20, 8, 2>"), (11, "k_drc<20, 8, 2>")):
        assert on.native.kernel_info(op) == off.native.kernel_info(op) == want
    r9 = recipe_synthetic(np.full((2, 2), .5), np.array([.5, .5]), 9, 9, 20, 8, seed=25)
    c9 = core.Cache(build_problem(r9)[1])
    assert c9.native.kernel_info(15) == ""
