"""GPU: the evaluation of a solve (Solver.evaluate / evaluate_batch, NativeContext.evaluate /
cp_batch_evaluate; k_eval_nodes, k_eval_sweep, k_eval_batch) against tests/eval_ref.py, the
float64 NumPy reference whose AVaR tests/test_eval_host.py pins on an LP solver.

Bounds. fp64: every node value within 1e-12 of the largest reference value (the suite's bound for
one operator application; AVaR is a convex combination, so the sweep does not amplify), s_0 exact,
the box and dynamics figures within 1e-12 max(1, |z|_inf). fp32 (values loaded as float, all
arithmetic double; the reference is float64 on the widened iterate with the unrounded tables):
4e-6 in place of 1e-12, the suite's 2e-6 for one fp32 operator application
(test_gpu_fp32.TOL32) doubled for the square.
"""
import contextlib
import os

import numpy as np
import pytest

import branch_cases as bc
import eval_ref
import raocp.core as core
from oracle.raocp_oracle import OracleProblem
from raocp.core._native import RaocpError
from raocp.problems import (build_problem, recipe_general, recipe_general_small, recipe_main, recipe_ops2x2,
                            recipe_synthetic)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = ["float64", "float32"]
TOL = {"float64": 1e-12, "float32": 4e-6}
_CHAIN = np.array([[0.1, 0.8, 0.1], [0.4, 0.6, 0.0], [0.0, 0.3, 0.7]])
_CHAIN_V = np.array([0.1, 0.6, 0.3])
_BIN = (np.full((2, 2), .5), np.full(2, .5))
_TERN = (np.full((3, 3), 1 / 3), np.full(3, 1 / 3))

RECIPES = {
    "main": recipe_main,
    "ops2x2": recipe_ops2x2,  # no boxes
    "g53": lambda: recipe_general_small("g53"),     # 27 nodes, 1 / 2 / 3 children, alpha 0.1, (5, 3)
    "g175": lambda: recipe_general_small("g175"),   # binary, (17, 5), alpha 0.7
    "g618": lambda: recipe_general_small("g618"),   # (6, 18), alpha 0.99
    "g53-max": lambda: recipe_general(_CHAIN, _CHAIN_V, 3, 3, 5, 3, seed=53, alpha_r=0.0),   # AVaR = maximum
    "g53-mean": lambda: recipe_general(_CHAIN, _CHAIN_V, 3, 3, 5, 3, seed=53, alpha_r=1.0),  # AVaR = expectation
    # 1,023 nodes: the deepest parent stages span several workgroups of the sweep, seven stages merge in its last launch
    "bin9": lambda: recipe_general(*_BIN, 9, 9, 5, 3, seed=9, alpha_r=0.7),
    "tern5": lambda: recipe_general(*_TERN, 5, 5, 17, 5, seed=5, alpha_r=0.7),               # 364 nodes
    "s64x32": lambda: bc._shape_recipe(64, 32, False),                                        # the largest admitted sizes
}
ARBITRARY = ["g53", "g175", "g618", "g53-max", "g53-mean", "bin9", "tern5", "s64x32"]
SWEEPS = {"bin9": 3, "tern5": 2, "g53": 1}  # launches of k_eval_sweep the plan predicts (64 parents per workgroup)

_PROB = {}


def _problem(name):
    """(recipe, problem, oracle) of a test problem, built once."""
    if name not in _PROB:
        r = RECIPES[name]()
        prob = build_problem(r)[1]
        _PROB[name] = (r, prob, OracleProblem(prob))
    return _PROB[name]


@contextlib.contextmanager
def env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    try:
        os.environ.update({k: str(v) for k, v in kv.items()})
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _held(x, dtype):
    """x as a context of dtype holds it."""
    x = np.asarray(x, dtype=np.float64)
    return x.astype(np.float32).astype(np.float64) if dtype == "float32" else x


def _golden_alpha():
    return float(np.load(os.path.join(ROOT, "tests", "golden", "main_trace.npz"))["main/cp_alpha"])


def _check(got4, vals, orc, z, x0, dtype, what=""):
    """The four figures (and the node values, when given) against eval_ref on the same z."""
    tol = TOL[dtype]
    cost, s0, box, dyn, V = eval_ref.evaluate(orc, z, x0)
    vmax, zmax = float(np.max(np.abs(V))), max(1.0, float(np.max(np.abs(z))))
    fig = dict(cost=abs(got4[0] - cost) / vmax, s0=abs(got4[1] - s0), box=abs(got4[2] - box) / zmax, dyn=abs(got4[3] - dyn) / zmax)
    if vals is not None:
        fig["nodes"] = float(np.max(np.abs(vals - V))) / vmax
    print(what, dtype, {k: f"{v:.2e}" for k, v in fig.items()}, f"cost {cost:.6g} box {box:.3g} dyn {dyn:.3g}")
    assert fig["s0"] == 0.0, fig
    assert all(v <= tol for k, v in fig.items() if k != "s0"), fig
    return cost, s0, box, dyn


# ---- 1. an arbitrary primal, every node

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ARBITRARY)
def test_arbitrary_primal_every_node(name, dtype):
    r, prob, orc = _problem(name)
    s = core.Solver(problem_spec=prob, dtype=dtype)
    nat = s.cache.native
    T = "float" if dtype == "float32" else "double"
    info = nat.kernel_info(17)
    assert info.startswith(f"k_eval_nodes<{T}> + k_eval_sweep<{T}> x")
    if name in SWEEPS:  # 6. the launch count the plan predicts
        assert info == f"k_eval_nodes<{T}> + k_eval_sweep<{T}> x{SWEEPS[name]}"
    if dtype == "float32" and max(s.cache.packed.sqrt_q.shape[0], s.cache.packed.sqrt_r.shape[0]) > 1:
        # a weight table per mode: an fp32 context refuses L itself, the evaluation works
        with pytest.raises(RaocpError, match="fp32 L / L\\^T need one weight table per node block"):
            nat.ell(np.zeros(nat.P))
    rng = np.random.default_rng(1000 + sum(map(ord, name)))
    z = np.where(orc.live_masks()[0], rng.standard_normal(orc.P), 0.0)
    x0 = np.asarray(r["x0"], dtype=float).reshape(-1)
    s.cache.cache_initial_state(x0.reshape(-1, 1))
    s.cache.set_primal_flat(z)
    held = nat.get_primal()
    assert np.array_equal(held, _held(z, dtype))
    ev = s.evaluate(node_values=True)
    assert ev.node_values.shape == (orc.n,)
    got = (ev.cost, ev.epigraph, ev.box_violation, ev.dynamics_residual)
    cost, s0, box, dyn = _check(got, ev.node_values, orc, held, _held(x0, dtype), dtype, name)
    assert cost > 0 and s0 != 0 and box > 0 and dyn > 0  # a random primal leaves none of them zero
    assert ev.cost == ev.node_values[0]
    # the same primal handed over from the host gives the same figures, and nothing has moved
    out = nat.evaluate(z)
    assert np.array_equal(out, np.array(got))
    assert np.array_equal(nat.get_primal(), held)
    assert s.evaluate().node_values is None


# ---- 2. exact cases

@pytest.mark.parametrize("dtype", DTYPES)
def test_zero_primal_costs_exactly_zero(dtype):
    """Every family ties at 0: the cost and every node value are exactly 0.0."""
    for name in ("main", "g53"):
        r, prob, orc = _problem(name)
        nat = core.Cache(prob, dtype=dtype).native
        nat.set_initial_state(np.zeros(orc.nx))
        nat.set_primal(np.zeros(orc.P))
        out, vals = nat.evaluate(node_values=True)
        assert out[0] == 0.0 and out[1] == 0.0 and out[3] == 0.0 and np.all(vals == 0.0), (name, out)


@pytest.mark.parametrize("dtype", DTYPES)
def test_nan_in_a_leaf_surfaces(dtype):
    r, prob, orc = _problem("main")
    nat = core.Cache(prob, dtype=dtype).native
    nat.set_initial_state(r["x0"])
    z = np.where(orc.live_masks()[0], np.random.default_rng(3).standard_normal(orc.P), 0.0)
    z[orc.X0 + (orc.n - 2) * orc.nx + 1] = np.nan
    out = nat.evaluate(z)
    assert np.isnan(out[0]) and np.isnan(out[2]) and np.isnan(out[3]), out
    assert out[1] == _held(z, dtype)[orc.S0]


@pytest.mark.parametrize("dtype", DTYPES)
def test_no_boxes_no_violation(dtype):
    r, prob, orc = _problem("ops2x2")
    assert not orc.nl_active.any() and not orc.l_active.any()
    nat = core.Cache(prob, dtype=dtype).native
    nat.set_initial_state(r["x0"])
    z = 10.0 * np.where(orc.live_masks()[0], np.random.default_rng(4).standard_normal(orc.P), 0.0)
    nat.set_primal(z)
    out, vals = nat.evaluate(node_values=True)
    assert out[2] == 0.0
    _check(out, vals, orc, nat.get_primal(), _held(r["x0"], dtype), dtype, "ops2x2")


# ---- 3. after a solve

def test_after_a_solve_main():
    """main.py's problem at its own tolerance: the recorded cost and s_0 (0.8 % apart), feasible."""
    r, prob, orc = _problem("main")
    s = core.Solver(problem_spec=prob)
    assert s.chock(r["x0"].reshape(-1, 1), max_iters=2000, tol=1e-3, step_size=_golden_alpha()) == 0
    ev = s.evaluate()
    print(ev)
    assert abs(ev.cost - 1.2522228374539) <= 1e-8 * 1.2522228374539
    assert abs(ev.epigraph - 1.2423913282094) <= 1e-8 * 1.2423913282094
    assert ev.dynamics_residual <= 1e-10
    assert ev.box_violation == 0.0
    _check((ev.cost, ev.epigraph, ev.box_violation, ev.dynamics_residual), None, orc, s.cache.get_primal_flat(), r["x0"],
           "float64", "main solved")


def test_after_a_solve_g53_cost_meets_epigraph():
    """3000 iterations at tol 0: converged, so V_0 equals s_0 (the oracle reaches 3.3e-14; the bound
    is the suite's 1e-10 iterate tolerance with a factor of ten for the quadratic)."""
    r, prob, orc = _problem("g53")
    s = core.Solver(problem_spec=prob)
    s.chock(r["x0"].reshape(-1, 1), max_iters=2999, tol=0.0)
    ev = s.evaluate()
    print(ev)
    assert abs(ev.cost - ev.epigraph) <= 1e-9 * abs(ev.cost)
    assert abs(ev.cost - 4.448456039332924) <= 1e-8 * 4.448456039332924


# ---- 4. batch

def _alpha(name):
    if name == "main":
        return _golden_alpha()
    return 0.999 / core.Cache(_problem(name)[1]).native.step_size()


def _batch_x0(name, B=5):
    r, prob, orc = _problem(name)
    rng = np.random.default_rng(77 + len(name))
    return np.asarray(r["x0"], dtype=float).reshape(1, -1) * rng.uniform(0.3, 1.2, (B, 1)) + 0.1 * rng.standard_normal((B, orc.nx))


def _check_batch(s, orc, X0, dtype, what):
    ev = s.evaluate_batch()
    B = X0.shape[0]
    assert ev.cost.shape == ev.epigraph.shape == ev.box_violation.shape == ev.dynamics_residual.shape == (B,)
    assert ev.node_values is None
    for b in range(B):
        got = (ev.cost[b], ev.epigraph[b], ev.box_violation[b], ev.dynamics_residual[b])
        _check(got, None, orc, s.batch_primal_flat(b), _held(X0[b], dtype), dtype, f"{what}[{b}]")
    return np.stack([ev.cost, ev.epigraph, ev.box_violation, ev.dynamics_residual], axis=1)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["main", "g53"])
def test_batch(name, dtype, monkeypatch):
    """evaluate_batch after chock_batch and after simulate_batch, on the batch kernel and on the
    sequential solves (RAOCP_CPB=0), and that it leaves everything as it was."""
    monkeypatch.setenv("RAOCP_CPB_F32", "1")
    r, prob, orc = _problem(name)
    alpha, X0 = _alpha(name), _batch_x0(name)
    T = "float" if dtype == "float32" else "double"
    s = core.Solver(problem_spec=prob, dtype=dtype)
    nat = s.cache.native
    assert nat.kernel_info(18) == f"k_eval_batch<{T}>"
    with pytest.raises(RaocpError, match="error -5"):
        s.evaluate_batch()
    s.chock_batch(X0, max_iters=50, tol=0.0, step_size=alpha)
    ctx_z = nat.get_primal()
    before = [(s.batch_primal_flat(b), s.batch_dual_flat(b)) for b in range(5)]
    fig = _check_batch(s, orc, X0, dtype, f"{name} batch")
    assert nat.kernel_info(18) == f"k_eval_batch<{T}>"
    # nothing moved: the slabs, the context's own primal, and a following warm batch
    assert np.array_equal(nat.get_primal(), ctx_z)
    for b in range(5):
        assert np.array_equal(s.batch_primal_flat(b), before[b][0]) and np.array_equal(s.batch_dual_flat(b), before[b][1])
    s.chock_batch(X0, max_iters=10, tol=0.0, step_size=alpha, warm=True)
    twin = core.Solver(problem_spec=prob, dtype=dtype)
    twin.chock_batch(X0, max_iters=50, tol=0.0, step_size=alpha)
    twin.chock_batch(X0, max_iters=10, tol=0.0, step_size=alpha, warm=True)
    for b in range(5):
        assert np.array_equal(s.batch_primal_flat(b), twin.batch_primal_flat(b))
        assert np.array_equal(s.batch_error_cache[b], twin.batch_error_cache[b])
    # after a closed-loop simulation: each instance's last solve, from the state it was solved from
    sim = s.simulate_batch(X0, 3, seed=5, max_iters=50, tol=0.0, step_size=alpha)
    _check_batch(s, orc, sim.states[:, 2], dtype, f"{name} mpc")
    # the sequential solves give the same values through the single-solve kernels
    with env(RAOCP_CPB=0):
        q = core.Solver(problem_spec=prob, dtype=dtype)
        assert q.cache.native.kernel_info(18) == ""
        q.chock_batch(X0, max_iters=50, tol=0.0, step_size=alpha)
        fig_seq = _check_batch(q, orc, X0, dtype, f"{name} batch seq")
        assert q.cache.native.kernel_info(18) == ""
        sim_q = q.simulate_batch(X0, 3, scenarios=sim.scenarios, max_iters=50, tol=0.0, step_size=alpha)
        _check_batch(q, orc, sim_q.states[:, 2], dtype, f"{name} mpc seq")
    # the two batches solve the same problems: their iterates agree to the suite's 1e-9 / 1e-5 of the
    # largest entry (test_gpu_batch.py, test_gpu_batch_fp32.py), the figures to ten times that
    scale = max(1.0, float(np.max(np.abs(before[0][0]))), float(np.max(np.abs(fig))))
    assert np.all(np.abs(fig - fig_seq) <= (1e-8 if dtype == "float64" else 1e-4) * scale), (fig, fig_seq)


# ---- 5. errors

def test_errors():
    r, prob, orc = _problem("main")
    s = core.Solver(problem_spec=prob)
    with pytest.raises(RaocpError, match="error -5.*initial state"):
        s.evaluate()
    with pytest.raises(RaocpError, match="error -5.*no batch"):
        s.evaluate_batch()
    # a sharded context refuses both
    rb = recipe_synthetic(*_BIN, 8, 8, 20, 8, seed=21)
    with env(RAOCP_DR=0, RAOCP_CP4=0, RAOCP_CP5=0, RAOCP_CP6=0):
        c = core.Cache(build_problem(rb)[1])
    c.native.set_initial_state(rb["x0"])
    c.native.evaluate()
    c.native.shard(0, 2)
    with pytest.raises(RaocpError, match="error -5.*sharded"):
        c.native.evaluate()
    with pytest.raises(RaocpError, match="error -5.*sharded"):
        c.native.cp_batch_evaluate()
