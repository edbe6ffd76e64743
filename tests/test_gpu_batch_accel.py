"""GPU: Anderson-accelerated batch solves (Solver.chock_batch(accel=m), raocp_cp_batch_run_aa,
k_cpa) against tests/accel_ref.py, the NumPy model over OracleProblem.cp_iteration.

Bounds. Against the oracle: 1e-8 per history entry and 1e-10 of the largest entry on the final
iterate, the bounds of tests/test_gpu_drc.py against the same oracle. gamma: the backward error
|Gbar gamma - b|_2 <= 1e-10 (|Gbar|_F |gamma|_2 + |b|_2); summation order and Cholesky rounding
are of order eps (P + D) m ~ 1e-12 here. Everything else is bit for bit.
"""
import contextlib
import os

import numpy as np
import pytest

import accel_ref
import eval_ref
import raocp.core as core
from oracle.raocp_oracle import OracleProblem
from helpers import problem_from_golden

pytestmark = pytest.mark.gpu

PROBLEMS = [("main_trace", "main"), ("traj_small", "c1n5"), ("traj_small", "ops2x2")]
_CACHE = {}


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


def _problem(golden, fixture, name):
    """The problem, its oracle, its pinned alpha and three distinct initial states (built once)."""
    if name not in _CACHE:
        z = golden(fixture)
        r, tree, prob = problem_from_golden(z, name)
        x0 = np.asarray(r["x0"], dtype=float).reshape(-1)
        _CACHE[name] = dict(prob=prob, orc=OracleProblem(prob), x0=x0, alpha=float(z[f"{name}/cp_alpha"]),
                            X=np.stack([x0, 0.5 * x0, -0.3 * x0]))
    return _CACHE[name]


def _main(golden):
    return _problem(golden, "main_trace", "main")


def _results(s, b):
    return (np.atleast_2d(s.batch_error_cache[b]), np.atleast_2d(s.batch_delta_error_cache[b]),
            s.batch_primal_flat(b), s.batch_dual_flat(b))


# ---- 1. off is off

@pytest.mark.parametrize("fixture,name", PROBLEMS)
def test_accel_zero_is_the_plain_solve_bitwise(golden, fixture, name):
    m = _problem(golden, fixture, name)
    a = core.Solver(problem_spec=m["prob"])
    b = core.Solver(problem_spec=m["prob"])
    sa = a.chock_batch(m["X"], max_iters=30, tol=0.0, step_size=m["alpha"])
    sb = b.chock_batch(m["X"], max_iters=30, tol=0.0, step_size=m["alpha"], accel=0)
    assert np.array_equal(sa, sb) and b.batch_accel_log == []
    assert np.array_equal(a.batch_first_inputs(), b.batch_first_inputs())
    for q in range(3):
        for x, y in zip(_results(a, q), _results(b, q)):
            assert np.array_equal(x, y)


# ---- 2. a rejection restores exactly

@pytest.mark.parametrize("fixture,name", PROBLEMS)
def test_rejection_restores_exactly(golden, fixture, name):
    m = _problem(golden, fixture, name)
    K = 60
    s = core.Solver(problem_spec=m["prob"])
    s.chock_batch(m["X"], max_iters=K, tol=0.0, step_size=m["alpha"], accel=5, accel_safeguard=0.0)
    plain = core.Solver(problem_spec=m["prob"])
    plain.chock_batch(m["X"], max_iters=K, tol=0.0, step_size=m["alpha"])
    for b in range(3):
        log = s.batch_accel_log[b]
        codes = log[:, 0].astype(int)
        assert log.shape == (K + 1, 12)
        assert 2 not in codes and np.count_nonzero(codes == 3) >= 10, codes   # every trial rejected
        assert codes[-1] != 3   # the last iteration is a plain one (a condition on K)
        keep = codes != 3
        n = int(np.count_nonzero(keep))
        err, derr, z, eta = _results(s, b)
        perr, pderr, _, _ = _results(plain, b)
        assert np.array_equal(err[keep], perr[:n]), b
        assert np.array_equal(derr[keep], pderr[:n]), b
        one = core.Solver(problem_spec=m["prob"])
        one.chock_batch(m["X"][b:b + 1], max_iters=n - 1, tol=0.0, step_size=m["alpha"])
        assert np.array_equal(z, one.batch_primal_flat(0)), b
        assert np.array_equal(eta, one.batch_dual_flat(0)), b


# ---- 3. replay against the oracle, 4. gamma solves what it should

@pytest.mark.parametrize("fixture,name", PROBLEMS)
def test_replay_against_the_oracle(golden, fixture, name):
    m = _problem(golden, fixture, name)
    K = 40
    s = core.Solver(problem_spec=m["prob"])
    s.chock_batch(m["X"], max_iters=K, tol=0.0, step_size=m["alpha"], accel=5)
    for b in range(3):
        log = s.batch_accel_log[b]
        codes = log[:, 0].astype(int)
        # conditions on the inputs (checked with the free model on the CPU first)
        assert np.count_nonzero(log[:, 2] == 1) >= 5 and np.count_nonzero(codes == 2) >= 1, codes
        ref = accel_ref.run(m["orc"], m["X"][b], m["alpha"], K, 0.0, m=5, log=log)
        err, derr, z, eta = _results(s, b)
        assert err.shape == ref.err.shape
        d_err = float(np.max(np.abs(err - ref.err)))
        d_derr = float(np.max(np.abs(derr - ref.derr)))
        d_z = float(np.max(np.abs(z - ref.z))) / float(np.max(np.abs(ref.z)))
        d_eta = float(np.max(np.abs(eta - ref.eta))) / max(float(np.max(np.abs(ref.eta))), 1e-300)
        d_log = float(np.max(np.abs(log[:, :4] - ref.log[:, :4]) / np.maximum(1.0, np.abs(ref.log[:, :4]))))
        print(name, b, "codes", np.bincount(codes, minlength=5), f"err {d_err:.2e} derr {d_derr:.2e} z {d_z:.2e} eta {d_eta:.2e} log {d_log:.2e}")
        assert d_err <= 1e-8 and d_derr <= 1e-8
        assert d_z <= 1e-10 and d_eta <= 1e-10
        # code, column count and what followed agree; |r|_2 within the history bound
        assert np.array_equal(log[:, :3], ref.log[:, :3])
        assert np.all(np.abs(log[:, 3] - ref.log[:, 3]) <= 1e-8 * np.maximum(1.0, ref.log[:, 3]))
        # every decision agrees with the model's own inequality unless the two sides are that close
        for k, lhs, rhs, code in ref.trials:
            if abs(lhs - rhs) > 1e-8 * max(lhs, rhs):
                assert code == (2 if lhs <= rhs else 3), (k, lhs, rhs, code)
        # 4. the backward error of every gamma on the model's own system
        assert len(ref.systems) >= 5
        worst = 0.0
        for k, Gb, bb, gam in ref.systems:
            res = float(np.linalg.norm(Gb @ gam - bb))
            bound = 1e-10 * (float(np.linalg.norm(Gb)) * float(np.linalg.norm(gam)) + float(np.linalg.norm(bb)))
            worst = max(worst, res / bound if bound > 0 else 0.0)
            assert res <= bound, (k, res, bound)
        print(name, b, f"gamma residual / bound {worst:.2e}")


# ---- 5. it converges where the plain solve does not

def test_converges_where_plain_does_not(golden):
    """The free model (tests/accel_ref.py, memory 5, a trial every iteration) needs 1,375 of the
    3,000 iterations on the CPU; plain CP has not converged after 3,000."""
    m = _main(golden)
    x0 = np.array([[2.0, -1.0, -1.0]])
    s = core.Solver(problem_spec=m["prob"])
    st = s.chock_batch(x0, max_iters=3000, tol=1e-5, accel=5)
    rows = np.atleast_2d(s.batch_error_cache[0])
    print("accelerated: status", st, "iterations", rows.shape[0], "codes", np.bincount(s.batch_accel_log[0][:, 0].astype(int), minlength=5))
    plain = core.Solver(problem_spec=m["prob"])
    sp = plain.chock_batch(x0, max_iters=3000, tol=1e-5)
    print("plain: status", sp, "last row", np.atleast_2d(plain.batch_error_cache[0])[-1])
    assert int(st[0]) == 0 and int(sp[0]) == 1
    assert rows.shape[0] < 3001 and float(np.max(rows[-1])) <= 1e-5
    # the fixed point is real: one oracle iteration from the pair the last one was computed from
    zp, ep = s.cache.native.cp_batch_get_prev(0)
    z1, e1, err, derr = m["orc"].cp_iteration(zp, ep, s.step_size, x0[0])
    print("last row", rows[-1], "oracle", err)
    assert np.all(np.abs(err - rows[-1]) <= 1e-8)
    assert np.all(np.abs(derr - np.atleast_2d(s.batch_delta_error_cache[0])[-1]) <= 1e-8)
    assert float(np.max(np.abs(z1 - s.batch_primal_flat(0)))) <= 1e-10 * float(np.max(np.abs(z1)))


# ---- 6. invariance

def _run_at(m, B, pos, chunk, K=30):
    rng = np.random.default_rng(5)
    X = m["x0"][None, :] * (0.05 + rng.random((B, 1))) + 0.01 * rng.standard_normal((B, m["x0"].size))
    for q in pos:
        X[q] = m["x0"]
    s = core.Solver(problem_spec=m["prob"])
    with env(RAOCP_BATCH_CHUNK=chunk):
        s.chock_batch(X, max_iters=K, tol=0.0, step_size=m["alpha"], accel=5)
    return [_results(s, q) + (s.batch_accel_log[q], s.batch_first_inputs()[q]) for q in pos]


def test_batch_position_and_chunk_invariance_bitwise(golden):
    m = _main(golden)
    ref = _run_at(m, 1, [0], 256)[0]
    assert np.count_nonzero(ref[4][:, 2] == 1) >= 5   # proposals, so chunk 1 splits them from their trials
    for chunk in (1, 7, 256):
        got = _run_at(m, 1, [0], chunk) + _run_at(m, 5, [3], chunk) + _run_at(m, 64, [0, 63], chunk)
        for g in got:
            for a, b in zip(g, ref):
                assert np.array_equal(a, b), chunk


# ---- 7. edges

def test_nan_isolation(golden):
    m = _main(golden)
    X = np.stack([m["x0"], 0.5 * m["x0"], 0.3 * m["x0"], 0.1 * m["x0"]])
    good = core.Solver(problem_spec=m["prob"])
    good.chock_batch(X, 30, 0.0, m["alpha"], accel=5)
    Xn = X.copy()
    Xn[2, 0] = np.nan
    s = core.Solver(problem_spec=m["prob"])
    with pytest.raises(ValueError) as ei:
        s.chock_batch(Xn, 30, 0.0, m["alpha"], accel=5)
    assert "[2]" in str(ei.value)
    for b in (0, 1, 3):
        for x, y in zip(_results(s, b), _results(good, b)):
            assert np.array_equal(x, y)
        assert np.array_equal(s.batch_accel_log[b], good.batch_accel_log[b])


def test_refusals_before_any_launch(golden):
    m = _main(golden)
    s = core.Solver(problem_spec=m["prob"])
    assert s.cache.native.kernel_info(19) in ("k_cpa<true>", "k_cpa<false>")
    for bad in (9, -1, 2.5):
        with pytest.raises(ValueError):
            s.chock_batch(m["X"], 5, 0.0, m["alpha"], accel=bad)
    with pytest.raises(ValueError):
        s.chock_batch(m["X"], 5, 0.0, m["alpha"], accel=5, accel_every=0)
    assert s.batch_error_cache == []   # nothing ran
    s32 = core.Solver(problem_spec=m["prob"], dtype="float32")
    assert s32.cache.native.kernel_info(19) == ""
    with pytest.raises(ValueError):
        s32.chock_batch(m["X"], 5, 0.0, m["alpha"], accel=5)
    with env(RAOCP_CPB=0):
        with pytest.raises(ValueError):
            s.chock_batch(m["X"], 5, 0.0, m["alpha"], accel=5)
    # a sharded context (the fixtures' trees are too small to shard: the benchmark tree, config 2)
    from raocp.problems import build_problem, recipe_config
    r2 = recipe_config(2, seed=0)
    sh = core.Solver(problem_spec=build_problem(r2)[1])
    sh.cache.native.shard(0, 2)
    with pytest.raises(ValueError):
        sh.chock_batch(np.zeros((2, np.asarray(r2["x0"]).size)), 1, 0.0, 0.1, accel=5)


def test_evaluate_and_warm_after_an_accelerated_solve(golden):
    """evaluate_batch against tests/eval_ref.py on the returned primal, with the bounds of
    tests/test_gpu_evaluate.py (fp64: 1e-12 of the largest node value / of max(1, |z|_inf), s_0
    exact); a warm batch afterwards starts with an empty history."""
    m = _main(golden)
    s = core.Solver(problem_spec=m["prob"])
    s.chock_batch(m["X"], 200, 0.0, m["alpha"], accel=5)
    ev = s.evaluate_batch()
    for b in range(3):
        z = s.batch_primal_flat(b)
        cost, s0, box, dyn, V = eval_ref.evaluate(m["orc"], z, m["X"][b])
        vmax, zmax = float(np.max(np.abs(V))), max(1.0, float(np.max(np.abs(z))))
        assert abs(ev.cost[b] - cost) <= 1e-12 * vmax
        assert ev.epigraph[b] == s0
        assert abs(ev.box_violation[b] - box) <= 1e-12 * zmax
        assert abs(ev.dynamics_residual[b] - dyn) <= 1e-12 * zmax
    s.chock_batch(m["X"], 10, 0.0, m["alpha"], warm=True, accel=5)
    for b in range(3):
        log = s.batch_accel_log[b]
        assert log.shape == (11, 12) and log[0, 0] == 0 and log[0, 1] == 0 and log[1, 2] == 1
