"""Closed-loop MPC simulation of a batch, resident on the device (Solver.simulate_batch,
raocp_cp_batch_mpc, k_mpc_step).

The central check replays every step from the device's own recorded state: k_cpb is bitwise
invariant to batch size, position and chunking (tests/test_gpu_batch.py), so step t of the
resident run must be bit-identical to chock_batch(states[:, t]) started from the replay's own
previous final iterate (warm) or from zero (t = 0, warm=False). Nothing compounds, so no
tolerance is needed. The plant step and the stage cost are compared with NumPy under
floating-point bounds of a dot product of that length evaluated in any order, with or without
FMA. Tolerances against the oracle and on the fallback paths are the project's
(tests/test_gpu_parity.py, tests/test_gpu_batch.py). Every problem comes from the committed
fixtures, except the sharded context of test_argument_errors."""
import contextlib
import os

import numpy as np
import pytest

import raocp.core as core
from raocp.core._native import RaocpError
from oracle.raocp_oracle import OracleProblem
from helpers import problem_from_golden, rel_err, trace_rel_err

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
FIXTURE = {"main": "main_trace", "bin6": "traj_small", "c1n5": "traj_small", "ops2x2": "traj_small"}
SCALES = (1.0, 0.5, 0.1, 0.0, 2.0)
# (instances, steps) of the replay cases
SHAPE = {"main": (5, 4), "bin6": (3, 3), "ops2x2": (3, 3), "c1n5": (3, 2)}


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


_PROB = {}


def _problem(golden, name):
    """A fixture problem, its pinned alpha, x0 and the root's children (built once)."""
    if name not in _PROB:
        z = golden(FIXTURE[name])
        r, tree, prob = problem_from_golden(z, name)
        _PROB[name] = dict(prob=prob, tree=tree, x0=np.asarray(r["x0"], dtype=float).reshape(-1),
                           alpha=float(z[f"{name}/cp_alpha"]), children=[int(i) for i in tree.children_of(0)])
    return _PROB[name]


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
        s = core.Solver(problem_spec=m["prob"])
        assert s.cache.native.kernel_info(14) == "k_mpc_step"
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
    """Every step of `res` against chock_batch from the recorded state; returns the replay
    solver's state after step 0 as (error caches, delta caches, primals) for the oracle check."""
    B, T = res.scenarios.shape
    rep = core.Solver(problem_spec=m["prob"])
    step0 = None
    for t in range(T):
        st = rep.chock_batch(res.states[:, t], max_iters=K, tol=tol, step_size=m["alpha"], warm=warm and t > 0)
        assert np.array_equal(res.status[:, t], st), t
        assert np.array_equal(res.iterations[:, t], _rows(rep, B)), t
        assert np.array_equal(res.errors[:, t], _last_rows(rep, B)), t
        assert np.array_equal(res.inputs[:, t], rep.batch_first_inputs()), t
        if t == 0:
            step0 = (list(rep.batch_error_cache), list(rep.batch_delta_error_cache),
                     [rep.batch_primal_flat(b) for b in range(B)])
    if fin is not None:
        for b in range(B):
            assert np.array_equal(fin[b][0], rep.batch_primal_flat(b)), b
            assert np.array_equal(fin[b][1], rep.batch_dual_flat(b)), b
        assert np.array_equal(first, rep.batch_first_inputs())
    return step0


def _assert_plant_and_cost(m, res):
    prob = m["prob"]
    B, T = res.scenarios.shape
    nx, nu = res.states.shape[2], res.inputs.shape[2]
    for b in range(B):
        for t in range(T):
            i = m["children"][int(res.scenarios[b, t])]
            A = np.asarray(prob.state_dynamics_at_node(i), dtype=float)
            Bm = np.asarray(prob.control_dynamics_at_node(i), dtype=float)
            x, u = res.states[b, t], res.inputs[b, t]
            bound = (nx + nu + 1) * EPS * (np.abs(A) @ np.abs(x) + np.abs(Bm) @ np.abs(u))
            diff = np.abs(res.states[b, t + 1] - (A @ x + Bm @ u))
            assert np.all(diff <= bound), (b, t, diff, bound)
            cost = prob.nonleaf_cost_at_node(i)
            SQ = np.asarray(cost.sqrt_state_weights, dtype=float)
            SR = np.asarray(cost.sqrt_control_weights, dtype=float)
            ref = float(np.sum((SQ @ x) ** 2) + np.sum((SR @ u) ** 2))
            cb = 1e-12 * float(np.sum((np.abs(SQ) @ np.abs(x)) ** 2) + np.sum((np.abs(SR) @ np.abs(u)) ** 2))
            assert abs(res.stage_costs[b, t] - ref) <= cb, (b, t, res.stage_costs[b, t], ref, cb)


_ORACLE = {}


def _oracle(m, name, K, X):
    if (name, K) not in _ORACLE:
        orc = OracleProblem(m["prob"])
        _ORACLE[(name, K)] = [orc.chock(x, K, 0.0, alpha=m["alpha"]) for x in X]
    return _ORACLE[(name, K)]


CASES = [(n, K) for n in ("main", "bin6", "ops2x2", "c1n5") for K in (29, 30, 31)]


@pytest.mark.parametrize("name,K", CASES)
def test_replay_bitwise_warm(golden, name, K):
    """max_iters 29 / 30 / 31 leave the final primal in rotation slots 0 / 1 / 2 and the final
    dual in slots 0 / 1 / 0: every move of the restart is taken."""
    m = _problem(golden, name)
    res, fin, first = _resident(golden, name, K, True)
    B, T = SHAPE[name]
    assert res.states.shape == (B, T + 1, m["x0"].size) and res.inputs.shape[:2] == (B, T)
    assert res.stage_costs.shape == res.status.shape == res.iterations.shape == (B, T) and res.errors.shape == (B, T, 3)
    assert np.array_equal(res.states[:, 0], _inputs(m, B, T)[0])
    assert np.all(res.iterations == K + 1) and np.all(res.status == 1)
    _assert_replay_bitwise(m, res, K, 0.0, True, fin, first)


@pytest.mark.parametrize("name,K", CASES)
def test_replay_bitwise_cold_and_oracle(golden, name, K):
    m = _problem(golden, name)
    res, fin, first = _resident(golden, name, K, False)
    B, T = SHAPE[name]
    errs, derrs, prim = _assert_replay_bitwise(m, res, K, 0.0, False, fin, first)
    # step 0 (bit-identical to the replay's) against the oracle
    for b, (st_o, err_o, derr_o, z_o, e_o, _) in enumerate(_oracle(m, name, K, res.states[:, 0])):
        assert int(res.status[b, 0]) == st_o
        assert trace_rel_err(errs[b], err_o) <= 1e-8
        assert trace_rel_err(derrs[b], derr_o) <= 1e-8
        assert trace_rel_err(res.errors[b, 0], err_o[-1]) <= 1e-8
        assert rel_err(prim[b], z_o) <= 1e-9


@pytest.mark.parametrize("name", ["main", "bin6", "ops2x2", "c1n5"])
@pytest.mark.parametrize("warm", [True, False])
def test_plant_step_and_cost(golden, name, warm):
    m = _problem(golden, name)
    for K in (29, 30, 31):
        res = _resident(golden, name, K, warm)[0]
        assert np.all(np.isfinite(res.states)) and np.all(np.isfinite(res.stage_costs))
        _assert_plant_and_cost(m, res)


def test_per_instance_stopping_inside_the_loop(golden):
    """Step 0's row counts are those of tests/test_gpu_batch.py::test_per_instance_stopping
    (937 / 980 for scales 1 / 0.5, 1001 rows and status 1 for scale 2)."""
    m = _problem(golden, "main")
    X = np.stack([sc * m["x0"] for sc in (1.0, 0.5, 2.0)])
    scen = np.array([[0, 1, 2], [1, 2, 0], [2, 0, 1]])
    s = core.Solver(problem_spec=m["prob"])
    with env(RAOCP_BATCH_CHUNK=16):
        res = s.simulate_batch(X, 3, scenarios=scen, max_iters=1000, tol=1e-3, step_size=m["alpha"])
        print("iterations", res.iterations.tolist(), "status", res.status.tolist())
        assert tuple(int(v) for v in res.iterations[:, 0]) == (937, 980, 1001)
        assert tuple(int(v) for v in res.status[:, 0]) == (0, 0, 1)
        fin = [(s.batch_primal_flat(b), s.batch_dual_flat(b)) for b in range(3)]
        _assert_replay_bitwise(m, res, 1000, 1e-3, True, fin, s.batch_first_inputs())
    # the instance that did not converge still advances
    assert np.all(res.iterations[2, 1:] > 0) and np.all(np.isfinite(res.states[2]))
    assert not np.array_equal(res.states[2, 1], res.states[2, 0])
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
    s = core.Solver(problem_spec=m["prob"])
    with env(RAOCP_BATCH_CHUNK=chunk):
        r = s.simulate_batch(X, T, scenarios=scen, max_iters=K, tol=0.0, step_size=m["alpha"])
    return [(r.states[q], r.inputs[q], r.stage_costs[q], r.status[q], r.iterations[q], r.errors[q],
             s.batch_primal_flat(q), s.batch_dual_flat(q), s.batch_first_inputs()[q]) for q in pos]


def test_chunk_batch_and_position_invariance_bitwise(golden):
    m = _problem(golden, "main")
    ref = _sim_at(m, 1, [0], 256)[0]
    for chunk in (7, 256):
        got = _sim_at(m, 1, [0], chunk) + _sim_at(m, 300, [0, 255, 256, 299], chunk)
        for g in got:
            for a, b in zip(g, ref):
                assert np.array_equal(a, b), chunk


def test_nan_isolation_and_freezing(golden):
    m = _problem(golden, "main")
    X = np.stack([m["x0"], 0.5 * m["x0"], 0.3 * m["x0"], 0.1 * m["x0"]])
    scen = np.array([[0, 1, 2], [1, 2, 0], [2, 0, 1], [1, 1, 0]])
    good = core.Solver(problem_spec=m["prob"])
    g = good.simulate_batch(X, 3, scenarios=scen, max_iters=30, tol=0.0, step_size=m["alpha"])
    Xn = X.copy()
    Xn[2, 0] = np.nan
    s = core.Solver(problem_spec=m["prob"])
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


def _assert_replay_close(m, s, res, K, dtype, ttol, ztol):
    """A fallback run against its own step-wise replay through chock_batch on the same path."""
    B, T = res.scenarios.shape
    rep = core.Solver(problem_spec=m["prob"], dtype=dtype)
    for t in range(T):
        st = rep.chock_batch(res.states[:, t], max_iters=K, tol=0.0, step_size=m["alpha"], warm=t > 0)
        assert np.array_equal(res.status[:, t], st) and np.array_equal(res.iterations[:, t], _rows(rep, B))
        assert trace_rel_err(res.errors[:, t], _last_rows(rep, B)) <= ttol
        assert rel_err(res.inputs[:, t], rep.batch_first_inputs()) <= ztol
    for b in range(B):
        assert rel_err(s.batch_primal_flat(b), rep.batch_primal_flat(b)) <= ztol
    _assert_plant_and_cost(m, res)


def test_fallback_and_untouched_context(golden):
    m = _problem(golden, "main")
    a = m["alpha"]
    X = np.stack([m["x0"], 0.5 * m["x0"], 0.1 * m["x0"]])
    scen = np.array([[0, 1], [1, 2], [2, 0]])
    ker = core.Solver(problem_spec=m["prob"])
    ker.chock(m["x0"].reshape(-1, 1), max_iters=5, tol=0.0, step_size=a)   # the context's own iterate
    z_before, e_before = ker.cache.native.get_primal(), ker.cache.native.get_dual()
    rk = ker.simulate_batch(X, 2, scenarios=scen, max_iters=40, tol=0.0, step_size=a)
    assert ker.cache.native.kernel_info(14) == "k_mpc_step"
    assert np.array_equal(ker.cache.native.get_primal(), z_before)
    assert np.array_equal(ker.cache.native.get_dual(), e_before)
    with env(RAOCP_CPB=0):
        seq = core.Solver(problem_spec=m["prob"])
        assert seq.cache.native.kernel_info(14) == ""
        seq.chock(m["x0"].reshape(-1, 1), max_iters=5, tol=0.0, step_size=a)
        z_before, e_before = seq.cache.native.get_primal(), seq.cache.native.get_dual()
        rs = seq.simulate_batch(X, 2, scenarios=scen, max_iters=40, tol=0.0, step_size=a)
        assert np.array_equal(seq.cache.native.get_primal(), z_before)
        assert np.array_equal(seq.cache.native.get_dual(), e_before)
        _assert_replay_close(m, seq, rs, 40, "float64", 1e-8, 1e-8)
        # the frozen rule of the host loop
        Xn = X.copy()
        Xn[1, 0] = np.nan
        with pytest.raises(ValueError):
            seq.simulate_batch(Xn, 2, scenarios=scen, max_iters=40, tol=0.0, step_size=a)
        rn = seq.batch_simulation
        assert np.all(rn.status[1] == 2) and rn.iterations[1, 1] == 0 and np.all(np.isnan(rn.states[1, 1:]))
        for b in (0, 2):
            assert np.array_equal(rn.states[b], rs.states[b]) and np.array_equal(rn.errors[b], rs.errors[b])
    # step 0 of the two paths solves the same problems
    assert np.array_equal(rk.status[:, 0], rs.status[:, 0])
    assert trace_rel_err(rs.errors[:, 0], rk.errors[:, 0]) <= 1e-8
    assert rel_err(rs.inputs[:, 0], rk.inputs[:, 0]) <= 1e-8
    # fp32: the host loop over the sequential solves
    s32 = core.Solver(problem_spec=m["prob"], dtype="float32")
    assert s32.cache.native.kernel_info(14) == ""
    r32 = s32.simulate_batch(X, 2, scenarios=scen, max_iters=40, tol=0.0, step_size=a)
    _assert_replay_close(m, s32, r32, 40, "float32", 1e-4, 1e-5)


def test_argument_errors(golden):
    m = _problem(golden, "main")
    nat = core.Cache(m["prob"]).native
    nx, nc, a = m["x0"].size, len(m["children"]), m["alpha"]
    with pytest.raises(RaocpError):
        nat.cp_batch_mpc(np.zeros((2, nx)), np.zeros((2, 0), dtype=np.int32), 1, 0.0, a)      # T = 0
    for B in (0, 4097):
        with pytest.raises(RaocpError):
            nat.cp_batch_mpc(np.zeros((B, nx)), np.zeros((B, 2), dtype=np.int32), 1, 0.0, a)
    bad = np.zeros((2, 2), dtype=np.int32)
    bad[1, 1] = nc
    with pytest.raises(RaocpError):
        nat.cp_batch_mpc(np.zeros((2, nx)), bad, 1, 0.0, a)
    bad[1, 1] = -1
    with pytest.raises(RaocpError):
        nat.cp_batch_mpc(np.zeros((2, nx)), bad, 1, 0.0, a)
    with pytest.raises(RaocpError):
        nat.cp_batch_mpc(np.zeros((2, nx)), np.zeros((2, 2), dtype=np.int32), -1, 0.0, a)
    # a sharded context (the fixtures' trees are too small to shard: the benchmark tree, config 2)
    from raocp.problems import build_problem, recipe_config
    r2 = recipe_config(2, seed=0)
    sh = core.Cache(build_problem(r2)[1]).native
    sh.shard(0, 2)
    with pytest.raises(RaocpError):
        sh.cp_batch_mpc(np.zeros((2, np.asarray(r2["x0"]).size)), np.zeros((2, 2), dtype=np.int32), 1, 0.0, 0.1)
    s = core.Solver(problem_spec=m["prob"])
    X = np.stack([m["x0"], 0.5 * m["x0"]])
    with pytest.raises(ValueError):
        s.simulate_batch(X, 3, scenarios=np.zeros((2, 4), dtype=np.int64), step_size=a)
    with pytest.raises(ValueError):
        s.simulate_batch(np.zeros((2, nx + 1)), 3, step_size=a)
    # the seeded sampler: the drawn paths are part of the result, and the run is reproducible
    r1 = s.simulate_batch(X, 5, seed=3, max_iters=20, tol=0.0, step_size=a)
    r2_ = core.Solver(problem_spec=m["prob"]).simulate_batch(X, 5, seed=3, max_iters=20, tol=0.0, step_size=a)
    assert r1.scenarios.shape == (2, 5) and np.array_equal(r1.scenarios, r2_.scenarios)
    for name in ("states", "inputs", "stage_costs", "status", "iterations", "errors"):
        assert np.array_equal(getattr(r1, name), getattr(r2_, name)), name
