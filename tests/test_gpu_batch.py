"""Batched Chambolle–Pock solves (Solver.chock_batch, raocp_cp_batch_run, k_cpb): many
initial states of one problem in one launch, one workgroup per instance.

Tolerances are the project's (tests/test_gpu_parity.py): 1e-8 relative per trace entry,
1e-9 on the final iterate. Every problem comes from the committed fixtures, except the sharded
context of test_argument_errors (the fixtures' trees are too small to shard)."""
import contextlib
import os

import numpy as np
import pytest

import raocp.core as core
from raocp.core._native import RaocpError
from oracle.raocp_oracle import OracleProblem
from helpers import problem_from_golden, rel_err, trace_rel_err

pytestmark = pytest.mark.gpu


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


_MAIN = {}


def _main(golden):
    """main.py's problem, its pinned alpha and x0 (built once)."""
    if not _MAIN:
        z = golden("main_trace")
        r, tree, prob = problem_from_golden(z, "main")
        _MAIN.update(z=z, prob=prob, x0=np.asarray(r["x0"], dtype=float).reshape(-1), alpha=float(z["main/cp_alpha"]))
    return _MAIN


@pytest.mark.parametrize("fixture,name", [("main_trace", "main"), ("traj_small", "bin6"), ("traj_small", "c1n5"),
                                          ("traj_small", "ops2x2")])
def test_golden_instance(golden, fixture, name):
    z = golden(fixture)
    r, tree, prob = problem_from_golden(z, name)
    x0 = np.asarray(r["x0"], dtype=float).reshape(-1)
    alpha = float(z[f"{name}/cp_alpha"])
    ref_err = z[f"{name}/cp_error"]
    max_iters, tol = int(z[f"{name}/cp_max_iters"]), float(z[f"{name}/cp_tol"])
    s = core.Solver(problem_spec=prob)
    assert s.cache.native.kernel_info(13) != ""
    X = np.stack([0.5 * x0, x0, 0.1 * x0])
    status = s.chock_batch(X, max_iters=max_iters, tol=tol, step_size=alpha)
    assert status.shape == (3,) and int(status[1]) == int(z[f"{name}/cp_status"])
    err = s.batch_error_cache[1]
    assert np.shape(err) == np.shape(ref_err)
    if name == "main":
        assert err.shape == (937, 3)
    print(name, "trace", trace_rel_err(err, ref_err), trace_rel_err(s.batch_delta_error_cache[1], z[f"{name}/cp_delta_error"]),
          "z", rel_err(s.batch_primal_flat(1), z[f"{name}/cp_z"]))
    assert trace_rel_err(err, ref_err) <= 1e-8
    assert trace_rel_err(s.batch_delta_error_cache[1], z[f"{name}/cp_delta_error"]) <= 1e-8
    assert rel_err(s.batch_primal_flat(1), z[f"{name}/cp_z"]) <= 1e-9
    if name == "main":
        assert rel_err(s.batch_dual_flat(1), z["main/cp_eta"]) <= 1e-9


@pytest.mark.parametrize("fixture,name", [("traj_small", "bin6"), ("main_trace", "main")])
def test_oracle_every_instance(golden, fixture, name):
    z = golden(fixture)
    r, tree, prob = problem_from_golden(z, name)
    x0 = np.asarray(r["x0"], dtype=float).reshape(-1)
    alpha = float(z[f"{name}/cp_alpha"])
    X = np.stack([x0, 0.5 * x0, 0.1 * x0, 0.0 * x0])
    s = core.Solver(problem_spec=prob)
    status = s.chock_batch(X, max_iters=30, tol=0.0, step_size=alpha)
    orc = OracleProblem(prob)
    u0 = s.batch_first_inputs()
    assert u0.shape == (4, orc.nu)
    for b in range(4):
        st_o, err_o, derr_o, z_o, e_o, _ = orc.chock(X[b], 30, 0.0, alpha=alpha)
        assert int(status[b]) == st_o == 1
        print(name, b, trace_rel_err(s.batch_error_cache[b], err_o), rel_err(s.batch_primal_flat(b), z_o))
        assert trace_rel_err(s.batch_error_cache[b], err_o) <= 1e-8
        assert trace_rel_err(s.batch_delta_error_cache[b], derr_o) <= 1e-8
        assert rel_err(s.batch_primal_flat(b), z_o) <= 1e-9
        assert np.array_equal(u0[b], s.batch_primal_flat(b)[orc.U0:orc.U0 + orc.nu])


def test_per_instance_stopping(golden):
    """Row counts 937 / 980 / 978 / 978 and the non-converging scale-2 run (1001 rows, status 1)
    were computed with the oracle on the CPU; every converging run's last error is <= 0.996 tol
    and the one before >= 1.004 tol, so no count sits on the threshold."""
    m = _main(golden)
    scales = (1.0, 0.5, 0.1, 0.0, 2.0)
    rows = (937, 980, 978, 978, 1001)
    stat = (0, 0, 0, 0, 1)
    X = np.stack([sc * m["x0"] for sc in scales])
    s = core.Solver(problem_spec=m["prob"])
    with env(RAOCP_BATCH_CHUNK=16):
        status = s.chock_batch(X, max_iters=1000, tol=1e-3, step_size=m["alpha"])
    got = tuple(int(np.atleast_2d(e).shape[0]) for e in s.batch_error_cache)
    print("rows", got, "status", status)
    assert got == rows
    assert tuple(int(v) for v in status) == stat
    for b in range(len(scales)):
        one = core.Solver(problem_spec=m["prob"])
        assert one.chock(X[b].reshape(-1, 1), max_iters=1000, tol=1e-3, step_size=m["alpha"]) == stat[b]
        assert trace_rel_err(s.batch_error_cache[b], one.error_cache) <= 1e-8
        assert trace_rel_err(s.batch_delta_error_cache[b], one.delta_error_cache) <= 1e-8


def _run_at(m, B, pos, chunk, K=20):
    """A batch of B distinct instances with main.py's x0 at the positions `pos`."""
    rng = np.random.default_rng(5)
    X = m["x0"][None, :] * (0.05 + rng.random((B, 1))) + 0.01 * rng.standard_normal((B, m["x0"].size))
    for q in pos:
        X[q] = m["x0"]
    s = core.Solver(problem_spec=m["prob"])
    with env(RAOCP_BATCH_CHUNK=chunk):
        s.chock_batch(X, max_iters=K, tol=0.0, step_size=m["alpha"])
    return [(s.batch_error_cache[q], s.batch_delta_error_cache[q], s.batch_primal_flat(q), s.batch_dual_flat(q))
            for q in pos]


def test_batch_and_position_invariance_bitwise(golden):
    m = _main(golden)
    ref = _run_at(m, 1, [0], 256)[0]
    for chunk in (1, 7, 256):
        got = _run_at(m, 1, [0], chunk) + _run_at(m, 7, [4], chunk) + _run_at(m, 300, [0, 255, 256, 299], chunk)
        for g in got:
            for a, b in zip(g, ref):
                assert np.array_equal(a, b), chunk


def test_contract_quirks(golden):
    m = _main(golden)
    z = m["z"]
    X = np.stack([m["x0"], m["x0"]])
    s = core.Solver(problem_spec=m["prob"])
    status = s.chock_batch(X, max_iters=0, tol=1e-3, step_size=m["alpha"])
    assert [int(v) for v in status] == [1, 1]
    for b in range(2):
        assert s.batch_error_cache[b].shape == (3,)
        assert trace_rel_err(s.batch_error_cache[b], z["main/cp_error"][0]) <= 1e-10
    # tol met exactly at k == max_iters returns 1
    status = s.chock_batch(X, max_iters=936, tol=1e-3, step_size=m["alpha"])
    assert [int(v) for v in status] == [1, 1]
    for b in range(2):
        assert s.batch_error_cache[b].shape == (937, 3)


def test_warm_start(golden):
    m = _main(golden)
    a = m["alpha"]
    X = np.stack([m["x0"], 0.5 * m["x0"], 0.1 * m["x0"]])
    s = core.Solver(problem_spec=m["prob"])
    s.chock_batch(X, 50, 0.0, a)
    s.chock_batch(X, 50, 0.0, a, warm=True)
    for b in range(3):
        one = core.Solver(problem_spec=m["prob"])
        one.chock(X[b].reshape(-1, 1), max_iters=50, tol=0.0, step_size=a)
        one.chock(X[b].reshape(-1, 1), max_iters=50, tol=0.0, step_size=a)
        assert trace_rel_err(s.batch_error_cache[b], one.error_cache) <= 1e-8
        assert trace_rel_err(s.batch_delta_error_cache[b], one.delta_error_cache) <= 1e-8
        assert rel_err(s.batch_primal_flat(b), one.cache.get_primal_flat()) <= 1e-9
    with pytest.raises(ValueError):
        s.chock_batch(X[:2], 50, 0.0, a, warm=True)


def test_nan_isolation(golden):
    m = _main(golden)
    X = np.stack([m["x0"], 0.5 * m["x0"], 0.3 * m["x0"], 0.1 * m["x0"]])
    good = core.Solver(problem_spec=m["prob"])
    good.chock_batch(X, 30, 0.0, m["alpha"])
    Xn = X.copy()
    Xn[2, 0] = np.nan
    s = core.Solver(problem_spec=m["prob"])
    with pytest.raises(ValueError) as ei:
        s.chock_batch(Xn, 30, 0.0, m["alpha"])
    assert "2" in str(ei.value) and "[2]" in str(ei.value)
    for b in (0, 1, 3):
        assert np.array_equal(s.batch_error_cache[b], good.batch_error_cache[b])
        assert np.array_equal(s.batch_delta_error_cache[b], good.batch_delta_error_cache[b])
        assert np.array_equal(s.batch_primal_flat(b), good.batch_primal_flat(b))
        assert np.array_equal(s.batch_dual_flat(b), good.batch_dual_flat(b))


def test_fallback_and_untouched_context(golden):
    m = _main(golden)
    a = m["alpha"]
    X = np.stack([m["x0"], 0.5 * m["x0"], 0.1 * m["x0"]])
    ker = core.Solver(problem_spec=m["prob"])
    ker.chock(m["x0"].reshape(-1, 1), max_iters=5, tol=0.0, step_size=a)   # the context's own iterate
    z_before, e_before = ker.cache.native.get_primal(), ker.cache.native.get_dual()
    st_k = ker.chock_batch(X, 40, 0.0, a)
    assert np.array_equal(ker.cache.native.get_primal(), z_before)
    assert np.array_equal(ker.cache.native.get_dual(), e_before)
    with env(RAOCP_CPB=0):
        seq = core.Solver(problem_spec=m["prob"])
        assert seq.cache.native.kernel_info(13) == ""
        seq.chock(m["x0"].reshape(-1, 1), max_iters=5, tol=0.0, step_size=a)
        z_before, e_before = seq.cache.native.get_primal(), seq.cache.native.get_dual()
        st_s = seq.chock_batch(X, 40, 0.0, a)
        assert np.array_equal(seq.cache.native.get_primal(), z_before)
        assert np.array_equal(seq.cache.native.get_dual(), e_before)
        assert np.array_equal(st_k, st_s)
        for b in range(3):
            assert trace_rel_err(seq.batch_error_cache[b], ker.batch_error_cache[b]) <= 1e-8
            assert trace_rel_err(seq.batch_delta_error_cache[b], ker.batch_delta_error_cache[b]) <= 1e-8
            assert rel_err(seq.batch_primal_flat(b), ker.batch_primal_flat(b)) <= 1e-8
        assert rel_err(seq.batch_first_inputs(), ker.batch_first_inputs()) <= 1e-8
    # fp32: the sequential solves, compared with the context's own single chock
    s32 = core.Solver(problem_spec=m["prob"], dtype="float32")
    assert s32.cache.native.kernel_info(13) == ""
    st32 = s32.chock_batch(X, 40, 0.0, a)
    for b in range(3):
        one = core.Solver(problem_spec=m["prob"], dtype="float32")
        assert one.chock(X[b].reshape(-1, 1), max_iters=40, tol=0.0, step_size=a) == int(st32[b])
        assert trace_rel_err(s32.batch_error_cache[b], one.error_cache) <= 1e-4
        assert trace_rel_err(s32.batch_delta_error_cache[b], one.delta_error_cache) <= 1e-4
        assert rel_err(s32.batch_primal_flat(b), one.cache.get_primal_flat()) <= 1e-5


def test_argument_errors(golden):
    m = _main(golden)
    nat = core.Cache(m["prob"]).native
    nx = m["x0"].size
    for B in (0, 4097):
        with pytest.raises(RaocpError):
            nat.cp_batch_run(np.zeros((B, nx)), 1, 0.0, m["alpha"])
    with pytest.raises(RaocpError):
        nat.cp_batch_get(0)   # no batch has been run
    # a sharded context (the fixtures' trees are too small to shard: the benchmark tree, config 2)
    from raocp.problems import build_problem, recipe_config
    r2 = recipe_config(2, seed=0)
    sh = core.Cache(build_problem(r2)[1]).native
    sh.shard(0, 2)
    with pytest.raises(RaocpError):
        sh.cp_batch_run(np.zeros((2, np.asarray(r2["x0"]).size)), 1, 0.0, 0.1)
    with pytest.raises(ValueError):
        core.Solver(problem_spec=m["prob"]).chock_batch(np.zeros((3, nx + 1)))
