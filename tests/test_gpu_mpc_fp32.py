"""Closed-loop MPC simulation of a batch on float32 contexts (Solver(problem,
dtype="float32").simulate_batch, k_cpb<float, .> and k_mpc_step<float>).

As in tests/test_gpu_mpc.py the central check replays every step from the device's own recorded
state: the float batch kernel is bitwise invariant to batch size, position and chunking
(tests/test_gpu_batch_fp32.py), the recorded states are floats widened to double, so step t of the
resident run must be bit-identical to chock_batch(states[:, t]) started from the replay's own
previous final iterate (warm) or from zero. Nothing compounds, so no tolerance is needed.

The plant step is computed in float from float operands: against NumPy in double on the
float-rounded operands it is within (nx + nu + 1) 2^-23 (|A||x| + |B||u|), the bound of a dot
product of that length in any order, with or without FMA, plus the final rounding. The stage cost
is within 1e-5 (|| |sqrt Q||x| ||^2 + || |sqrt R||u| ||^2), the project's fp32 iterate bound."""
import contextlib
import os

import numpy as np
import pytest

import raocp.core as core
from helpers import problem_from_golden

pytestmark = pytest.mark.gpu

EPS32 = 2.0 ** -23
FIXTURE = {"main": "main_trace", "c1n5": "traj_small", "ops2x2": "traj_small"}
SCALES = (1.0, 0.5, 0.1, 0.0, 2.0)
# (instances, steps) of the replay cases
SHAPE = {"main": (5, 4), "ops2x2": (3, 3), "c1n5": (3, 2)}


@contextlib.contextmanager
def env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    try:
        for k, v in kv.items():
            os.environ[k] = str(v)
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(autouse=True)
def _float_kernels(monkeypatch):
    """An fp32 context takes the float kernels when RAOCP_CPB_F32=1 (read at call time); without
    it an fp32 context keeps the host loop over sequential solves (tests/test_gpu_mpc.py pins
    kernel_info(14) == "" on a default fp32 context)."""
    monkeypatch.setenv("RAOCP_CPB_F32", "1")


_PROB = {}


def _problem(golden, name):
    if name not in _PROB:
        z = golden(FIXTURE[name])
        r, tree, prob = problem_from_golden(z, name)
        _PROB[name] = dict(prob=prob, tree=tree, x0=np.asarray(r["x0"], dtype=float).reshape(-1),
                           alpha=float(z[f"{name}/cp_alpha"]), children=[int(i) for i in tree.children_of(0)])
    return _PROB[name]


def _solver32(m):
    return core.Solver(problem_spec=m["prob"], dtype="float32")


def _inputs(m, B, T):
    """B scaled copies of the fixture's x0 and scenario paths that cover every root child."""
    X = np.stack([SCALES[b] * m["x0"] for b in range(B)])
    nc = len(m["children"])
    scen = np.array([[(b + t) % nc for t in range(T)] for b in range(B)], dtype=np.int64)
    assert set(scen.reshape(-1)) == set(range(nc))
    return X, scen


_RUNS = {}


def _resident(golden, name, K, warm):
    """The resident run of a replay case with its final iterates (computed once, not modified)."""
    key = (name, K, warm)
    if key not in _RUNS:
        m = _problem(golden, name)
        B, T = SHAPE[name]
        X, scen = _inputs(m, B, T)
        s = _solver32(m)
        assert s.cache.native.kernel_info(14) == "k_mpc_step<float>"
        res = s.simulate_batch(X, T, scenarios=scen, max_iters=K, tol=0.0, step_size=m["alpha"], warm=warm)
        assert res is s.batch_simulation
        fin = [(s.batch_primal_flat(b), s.batch_dual_flat(b)) for b in range(B)]
        _RUNS[key] = (res, fin, s.batch_first_inputs())
    return _RUNS[key]


def _last_rows(solver, B):
    return np.stack([np.atleast_2d(solver.batch_error_cache[b])[-1] for b in range(B)])


def _rows(solver, B):
    return np.array([np.atleast_2d(solver.batch_error_cache[b]).shape[0] for b in range(B)])


def _assert_replay_bitwise(m, res, K, tol, warm, fin=None, first=None):
    B, T = res.scenarios.shape
    rep = _solver32(m)
    for t in range(T):
        st = rep.chock_batch(res.states[:, t], max_iters=K, tol=tol, step_size=m["alpha"], warm=warm and t > 0)
        assert np.array_equal(res.status[:, t], st), t
        assert np.array_equal(res.iterations[:, t], _rows(rep, B)), t
        assert np.array_equal(res.errors[:, t], _last_rows(rep, B)), t
        assert np.array_equal(res.inputs[:, t], rep.batch_first_inputs()), t
    if fin is not None:
        for b in range(B):
            assert np.array_equal(fin[b][0], rep.batch_primal_flat(b)), b
            assert np.array_equal(fin[b][1], rep.batch_dual_flat(b)), b
        assert np.array_equal(first, rep.batch_first_inputs())


def _f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def _assert_plant_and_cost(m, res):
    prob = m["prob"]
    B, T = res.scenarios.shape
    nx, nu = res.states.shape[2], res.inputs.shape[2]
    worst_x = worst_c = 0.0
    for b in range(B):
        for t in range(T):
            i = m["children"][int(res.scenarios[b, t])]
            A = _f32(prob.state_dynamics_at_node(i))
            Bm = _f32(prob.control_dynamics_at_node(i))
            x, u = res.states[b, t], res.inputs[b, t]
            assert np.array_equal(x, _f32(x)) and np.array_equal(u, _f32(u))
            bound = (nx + nu + 1) * EPS32 * (np.abs(A) @ np.abs(x) + np.abs(Bm) @ np.abs(u))
            diff = np.abs(res.states[b, t + 1] - (A @ x + Bm @ u))
            worst_x = max(worst_x, float(np.max(diff / np.maximum(bound, 1e-300))))
            assert np.all(diff <= bound), (b, t, diff, bound)
            cost = prob.nonleaf_cost_at_node(i)
            SQ = _f32(cost.sqrt_state_weights)
            SR = _f32(cost.sqrt_control_weights)
            ref = float(np.sum((SQ @ x) ** 2) + np.sum((SR @ u) ** 2))
            cb = 1e-5 * float(np.sum((np.abs(SQ) @ np.abs(x)) ** 2) + np.sum((np.abs(SR) @ np.abs(u)) ** 2))
            worst_c = max(worst_c, abs(res.stage_costs[b, t] - ref) / max(cb, 1e-300))
            assert abs(res.stage_costs[b, t] - ref) <= cb, (b, t, res.stage_costs[b, t], ref, cb)
    print("plant step: worst |diff| / bound %.3f; stage cost: worst |diff| / bound %.3f" % (worst_x, worst_c))


CASES = [(n, K) for n in ("main", "ops2x2", "c1n5") for K in (29, 30, 31)]


@pytest.mark.parametrize("name,K", CASES)
def test_replay_bitwise_warm(golden, name, K):
    """max_iters 29 / 30 / 31 leave the final primal in rotation slots 0 / 1 / 2 and the final
    dual in slots 0 / 1 / 0: every move of the restart is taken."""
    m = _problem(golden, name)
    res, fin, first = _resident(golden, name, K, True)
    B, T = SHAPE[name]
    assert res.states.shape == (B, T + 1, m["x0"].size) and res.inputs.shape[:2] == (B, T)
    assert res.stage_costs.shape == res.status.shape == res.iterations.shape == (B, T) and res.errors.shape == (B, T, 3)
    for arr in (res.states, res.inputs, res.stage_costs, res.errors):
        assert arr.dtype == np.float64
    assert res.status.dtype == res.iterations.dtype == np.int64
    assert np.array_equal(res.states[:, 0], _f32(_inputs(m, B, T)[0]))
    assert np.all(res.iterations == K + 1) and np.all(res.status == 1)
    _assert_replay_bitwise(m, res, K, 0.0, True, fin, first)


@pytest.mark.parametrize("name,K", CASES)
def test_replay_bitwise_cold(golden, name, K):
    m = _problem(golden, name)
    res, fin, first = _resident(golden, name, K, False)
    _assert_replay_bitwise(m, res, K, 0.0, False, fin, first)


@pytest.mark.parametrize("name", ["main", "ops2x2", "c1n5"])
@pytest.mark.parametrize("warm", [True, False])
def test_plant_step_and_cost(golden, name, warm):
    m = _problem(golden, name)
    for K in (29, 30, 31):
        res = _resident(golden, name, K, warm)[0]
        assert np.all(np.isfinite(res.states)) and np.all(np.isfinite(res.stage_costs))
        _assert_plant_and_cost(m, res)


def _sim_at(m, B, pos, chunk, K=20, T=3):
    """A batch of B distinct instances with the fixture's x0 and one scenario path at `pos`."""
    rng = np.random.default_rng(5)
    nc = len(m["children"])
    X = m["x0"][None, :] * (0.05 + rng.random((B, 1))) + 0.01 * rng.standard_normal((B, m["x0"].size))
    scen = rng.integers(0, nc, size=(B, T))
    for q in pos:
        X[q] = m["x0"]
        scen[q] = [t % nc for t in range(T)]
    s = _solver32(m)
    with env(RAOCP_BATCH_CHUNK=chunk):
        r = s.simulate_batch(X, T, scenarios=scen, max_iters=K, tol=0.0, step_size=m["alpha"])
    return [(r.states[q], r.inputs[q], r.stage_costs[q], r.status[q], r.iterations[q], r.errors[q],
             s.batch_primal_flat(q), s.batch_dual_flat(q), s.batch_first_inputs()[q]) for q in pos]


def test_chunk_batch_and_position_invariance_bitwise(golden):
    m = _problem(golden, "main")
    ref = _sim_at(m, 1, [0], 256)[0]
    assert np.all(np.isfinite(ref[0])) and not np.array_equal(ref[0][1], ref[0][0])
    for chunk in (7, 256):
        got = _sim_at(m, 1, [0], chunk) + _sim_at(m, 300, [0, 255, 256, 299], chunk)
        for g in got:
            for a, b in zip(g, ref):
                assert np.array_equal(a, b), chunk


def test_nan_isolation_and_freezing(golden):
    m = _problem(golden, "main")
    X = np.stack([m["x0"], 0.5 * m["x0"], 0.3 * m["x0"], 0.1 * m["x0"]])
    scen = np.array([[0, 1, 2], [1, 2, 0], [2, 0, 1], [1, 1, 0]])
    good = _solver32(m)
    g = good.simulate_batch(X, 3, scenarios=scen, max_iters=30, tol=0.0, step_size=m["alpha"])
    Xn = X.copy()
    Xn[2, 0] = np.nan
    s = _solver32(m)
    with pytest.raises(ValueError) as ei:
        s.simulate_batch(Xn, 3, scenarios=scen, max_iters=30, tol=0.0, step_size=m["alpha"])
    assert "instances [2]" in str(ei.value) and "steps [0]" in str(ei.value)
    r = s.batch_simulation
    assert np.all(r.status[2] == 2) and r.iterations[2, 0] > 0 and np.all(r.iterations[2, 1:] == 0)
    assert np.all(np.isnan(r.states[2, 1:])) and np.all(np.isnan(r.inputs[2])) and np.all(np.isnan(r.stage_costs[2]))
    for b in (0, 1, 3):
        for a, c in ((r.states, g.states), (r.inputs, g.inputs), (r.stage_costs, g.stage_costs), (r.status, g.status),
                     (r.iterations, g.iterations), (r.errors, g.errors)):
            assert np.array_equal(a[b], c[b]), b
        assert np.array_equal(s.batch_primal_flat(b), good.batch_primal_flat(b))
        assert np.array_equal(s.batch_dual_flat(b), good.batch_dual_flat(b))
