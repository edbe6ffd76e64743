"""Batched Chambolle–Pock solves on float32 contexts (Solver(problem, dtype="float32").chock_batch,
k_cpb<float, .>): the float form of the batch kernel, one workgroup per instance.

Bitwise checks need no tolerance. The others use the project's fp32 bounds
(tests/test_gpu_fp32.py::test_fp32_mixed_weight_tables_ops2x2): 1e-4 per trace entry
(trace_rel_err) and 1e-5 of the largest entry on the iterate (rel_err). The problems are the small
fixtures the fp64 batch tests use: main.py's 43-node tree (ragged 1 / 2 / 3 children, single-child
stages, boxes), c1n5 and ops2x2 (a different sqrt Q / sqrt R table per mode, no boxes).

An fp32 context takes the float kernel when RAOCP_CPB_F32=1 (read at call time); without it an
fp32 context keeps the sequential solves it has always run, which tests/test_gpu_batch.py pins
(kernel_info(13) == "" on a default fp32 context). Every test here runs with the switch set;
test_selection also checks the default."""
import contextlib
import os

import numpy as np
import pytest

import raocp.core as core
from oracle.raocp_oracle import OracleProblem
from helpers import problem_from_golden, rel_err, trace_rel_err

pytestmark = pytest.mark.gpu

TRACE_TOL, Z_TOL = 1e-4, 1e-5
FIXTURE = {"main": "main_trace", "c1n5": "traj_small", "ops2x2": "traj_small"}
SCALES = (1.0, 0.5, 0.1)
K = 29


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
def _float_kernel(monkeypatch):
    monkeypatch.setenv("RAOCP_CPB_F32", "1")


_PROB = {}


def _problem(golden, name):
    """A fixture problem, its pinned alpha and x0 (built once)."""
    if name not in _PROB:
        z = golden(FIXTURE[name])
        r, tree, prob = problem_from_golden(z, name)
        _PROB[name] = dict(prob=prob, x0=np.asarray(r["x0"], dtype=float).reshape(-1), alpha=float(z[f"{name}/cp_alpha"]))
    return _PROB[name]


def _solver32(m):
    return core.Solver(problem_spec=m["prob"], dtype="float32")


def _state(s, b):
    return (s.batch_error_cache[b], s.batch_delta_error_cache[b], s.batch_primal_flat(b), s.batch_dual_flat(b))


_RUNS = {}


def _kernel_run(golden, name):
    """K = 29, tol = 0, pinned alpha on the batch kernel: per instance (err, derr, z, eta), and the
    first inputs (computed once, not modified)."""
    if name not in _RUNS:
        m = _problem(golden, name)
        X = np.stack([sc * m["x0"] for sc in SCALES])
        s = _solver32(m)
        assert s.cache.native.kernel_info(13).startswith("k_cpb<float")
        status = s.chock_batch(X, max_iters=K, tol=0.0, step_size=m["alpha"])
        _RUNS[name] = (X, status, [_state(s, b) for b in range(len(SCALES))], s.batch_first_inputs())
    return _RUNS[name]


def test_selection(golden):
    m = _problem(golden, "main")
    s32 = _solver32(m)
    assert s32.cache.native.kernel_info(13) in ("k_cpb<float, true>", "k_cpb<float, false>")
    assert s32.cache.native.kernel_info(14) == "k_mpc_step<float>"
    with env(RAOCP_CPB=0):
        assert s32.cache.native.kernel_info(13) == "" and s32.cache.native.kernel_info(14) == ""
    # without the switch an fp32 context keeps its sequential solves
    for off in ("0", ""):
        with env(RAOCP_CPB_F32=off):
            assert s32.cache.native.kernel_info(13) == "" and s32.cache.native.kernel_info(14) == ""
    s64 = core.Solver(problem_spec=m["prob"])
    for f32_switch in ("1", "0"):
        with env(RAOCP_CPB_F32=f32_switch):
            assert s64.cache.native.kernel_info(13) in ("k_cpb<true>", "k_cpb<false>")
            assert s64.cache.native.kernel_info(14) == "k_mpc_step"
            with env(RAOCP_CPB=0):
                assert s64.cache.native.kernel_info(13) == "" and s64.cache.native.kernel_info(14) == ""
    # what the batch returns on an fp32 context: the types, shapes and dtypes of an fp64 one
    X = np.stack([m["x0"], 0.5 * m["x0"]])
    for s in (s32, s64):
        st = s.chock_batch(X, max_iters=3, tol=0.0, step_size=m["alpha"])
        assert st.shape == (2,) and st.dtype == np.int64
        assert s.batch_error_cache[0].shape == (4, 3) and s.batch_error_cache[0].dtype == np.float64
        assert s.batch_delta_error_cache[1].shape == (4, 3)
        z, e, u = s.batch_primal_flat(1), s.batch_dual_flat(1), s.batch_first_inputs()
        assert z.dtype == e.dtype == u.dtype == np.float64 and u.shape == (2, 2)
        assert z.shape == s64.cache.get_primal_flat().shape
    # an fp32 context's values are floats widened to double
    z32 = s32.batch_primal_flat(0)
    assert np.array_equal(z32, z32.astype(np.float32).astype(np.float64))


def test_default_fp32_context_runs_what_it_ran(golden, monkeypatch):
    """Without the switch an fp32 chock_batch is the sequential solves."""
    monkeypatch.delenv("RAOCP_CPB_F32")
    m = _problem(golden, "main")
    X = np.stack([m["x0"], 0.5 * m["x0"]])
    dflt = _solver32(m)
    assert dflt.cache.native.kernel_info(13) == ""
    dflt.chock_batch(X, max_iters=10, tol=0.0, step_size=m["alpha"])
    with env(RAOCP_CPB=0):
        seq = _solver32(m)
        seq.chock_batch(X, max_iters=10, tol=0.0, step_size=m["alpha"])
        for b in range(2):
            d, q = _state(dflt, b), _state(seq, b)
            assert d[0].shape == q[0].shape == (11, 3)
            assert trace_rel_err(d[0], q[0]) <= TRACE_TOL and trace_rel_err(d[1], q[1]) <= TRACE_TOL
            assert rel_err(d[2], q[2]) <= Z_TOL and rel_err(d[3], q[3]) <= Z_TOL


def _run_at(m, B, pos, chunk, max_iters=20):
    """A batch of B distinct instances with the fixture's x0 at the positions `pos`."""
    rng = np.random.default_rng(5)
    X = m["x0"][None, :] * (0.05 + rng.random((B, 1))) + 0.01 * rng.standard_normal((B, m["x0"].size))
    for q in pos:
        X[q] = m["x0"]
    s = _solver32(m)
    with env(RAOCP_BATCH_CHUNK=chunk):
        s.chock_batch(X, max_iters=max_iters, tol=0.0, step_size=m["alpha"])
    u0 = s.batch_first_inputs()
    return [_state(s, q) + (u0[q],) for q in pos]


def test_batch_position_and_chunk_invariance_bitwise(golden):
    m = _problem(golden, "main")
    ref = _run_at(m, 1, [0], 256)[0]
    assert np.all(np.isfinite(ref[2])) and np.max(np.abs(ref[2])) > 0
    for chunk in (7, 256):
        got = _run_at(m, 1, [0], chunk) + _run_at(m, 300, [0, 255, 256, 299], chunk)
        for g in got:
            for a, b in zip(g, ref):
                assert np.array_equal(a, b), chunk


@pytest.mark.parametrize("max_iters", [0, 1, 2])
def test_contract_quirks_bitwise(golden, max_iters):
    """max_iters = k runs k + 1 iterations and reports status 1 even when tol is met at the last
    one; the one-row cache is 1-D. Alone and inside a batch, in one chunk or in chunks of 1."""
    m = _problem(golden, "main")
    ref = _run_at(m, 1, [0], 256, max_iters)[0]
    assert np.atleast_2d(ref[0]).shape == (max_iters + 1, 3)
    assert ref[0].ndim == (1 if max_iters == 0 else 2)
    for g in _run_at(m, 300, [0, 299], 256, max_iters) + _run_at(m, 3, [1], 1, max_iters):
        for a, b in zip(g, ref):
            assert np.array_equal(a, b)
    s = _solver32(m)
    status = s.chock_batch(np.stack([m["x0"], m["x0"]]), max_iters=max_iters, tol=1e30, step_size=m["alpha"])
    assert [int(v) for v in status] == ([1, 1] if max_iters == 0 else [0, 0])
    assert np.atleast_2d(s.batch_error_cache[0]).shape[0] == 1


@pytest.mark.parametrize("name", ["main", "c1n5", "ops2x2"])
def test_against_fp32_sequential_fallback(golden, name):
    """The same fp32 context type with RAOCP_CPB=0 runs k_cpd / k_cpp<float> and the fp32
    per-stage dynamics, which sum in another order: close, not bitwise."""
    m = _problem(golden, name)
    X, status, ker, u0 = _kernel_run(golden, name)
    with env(RAOCP_CPB=0):
        seq = _solver32(m)
        assert seq.cache.native.kernel_info(13) == ""
        st = seq.chock_batch(X, max_iters=K, tol=0.0, step_size=m["alpha"])
        assert np.array_equal(st, status)
        for b in range(len(SCALES)):
            figs = (trace_rel_err(ker[b][0], seq.batch_error_cache[b]), trace_rel_err(ker[b][1], seq.batch_delta_error_cache[b]),
                    rel_err(ker[b][2], seq.batch_primal_flat(b)), rel_err(ker[b][3], seq.batch_dual_flat(b)))
            print(name, b, "kernel vs fallback: err %.3e derr %.3e z %.3e eta %.3e" % figs)
            assert figs[0] <= TRACE_TOL and figs[1] <= TRACE_TOL
            assert figs[2] <= Z_TOL and figs[3] <= Z_TOL
        assert rel_err(u0, seq.batch_first_inputs()) <= Z_TOL


_ORACLE = {}


def _oracle(m, name, X):
    if name not in _ORACLE:
        orc = OracleProblem(m["prob"])
        _ORACLE[name] = [orc.chock(x, K, 0.0, alpha=m["alpha"]) for x in X]
    return _ORACLE[name]


@pytest.mark.parametrize("name", ["main", "c1n5", "ops2x2"])
def test_against_fp64_oracle(golden, name):
    """Several initial states per problem against OracleProblem.chock (fp64), K = 29, tol = 0,
    with the project's fp32 bounds as they stand: 1e-4 per trace entry, 1e-5 on the iterate. The
    fp32 sequential fallback (the code an fp32 chock_batch ran before the float kernel) is
    measured against the same oracle in the same test and printed beside the kernel's figures;
    it has to meet the same bounds."""
    m = _problem(golden, name)
    X, status, ker, u0 = _kernel_run(golden, name)
    ref = _oracle(m, name, X)
    with env(RAOCP_CPB=0):
        seq = _solver32(m)
        seq.chock_batch(X, max_iters=K, tol=0.0, step_size=m["alpha"])
        fall = [_state(seq, b) for b in range(len(SCALES))]
    orc = OracleProblem(m["prob"])
    for b, (st_o, err_o, derr_o, z_o, e_o, _) in enumerate(ref):
        assert int(status[b]) == st_o == 1
        for who, got in (("fallback", fall[b]), ("kernel", ker[b])):
            figs = (trace_rel_err(got[0], err_o), trace_rel_err(got[1], derr_o), rel_err(got[2], z_o), rel_err(got[3], e_o))
            print(name, b, who, "vs oracle: err %.3e derr %.3e z %.3e eta %.3e" % figs)
        for got in (fall[b], ker[b]):
            assert trace_rel_err(got[0], err_o) <= TRACE_TOL
            assert trace_rel_err(got[1], derr_o) <= TRACE_TOL
            assert rel_err(got[2], z_o) <= Z_TOL
            assert rel_err(got[3], e_o) <= Z_TOL
        assert np.array_equal(u0[b], ker[b][2][orc.U0:orc.U0 + orc.nu])


def test_per_instance_stopping(golden):
    m = _problem(golden, "main")
    tol, max_iters = 1e-3, 1200
    scales = (1.0, 0.5, 0.1, 0.0, 2.0)
    X = np.stack([sc * m["x0"] for sc in scales])
    s = _solver32(m)
    with env(RAOCP_BATCH_CHUNK=16):
        status = s.chock_batch(X, max_iters=max_iters, tol=tol, step_size=m["alpha"])
    rows = [int(np.atleast_2d(e).shape[0]) for e in s.batch_error_cache]
    print("rows", rows, "status", status)
    assert len(set(rows)) > 1 and int(np.sum(status == 0)) >= 3
    for b in range(len(scales)):
        err = np.atleast_2d(s.batch_error_cache[b])
        final_k = rows[b] - 1
        assert int(status[b]) == (0 if final_k < max_iters else 1)
        assert np.max(err[final_k - 1]) > tol
        if status[b] == 0:
            assert np.max(err[final_k]) <= tol
        one = _solver32(m)
        st1 = one.chock_batch(X[b:b + 1], max_iters=max_iters, tol=tol, step_size=m["alpha"])
        assert int(st1[0]) == int(status[b])
        for a, c in zip(_state(one, 0), _state(s, b)):
            assert np.array_equal(a, c), b


def test_nan_isolation(golden):
    m = _problem(golden, "main")
    X = np.stack([sc * m["x0"] for sc in (1.0, 0.5, 0.3, 0.1, 0.7)])
    good = _solver32(m)
    good.chock_batch(X, 30, 0.0, m["alpha"])
    Xn = X.copy()
    Xn[2, 0] = np.nan
    s = _solver32(m)
    with pytest.raises(ValueError) as ei:
        s.chock_batch(Xn, 30, 0.0, m["alpha"])
    assert "[2]" in str(ei.value)
    for b in (0, 1, 3, 4):
        for a, c in zip(_state(s, b), _state(good, b)):
            assert np.array_equal(a, c), b


def test_warm_start(golden):
    """K iterations, then a warm batch of K more, against one run of 2K + 1: the warm run starts
    from the first run's final iterate, which is where the long run stands after K + 1 rows."""
    m = _problem(golden, "main")
    a, k = m["alpha"], 20
    X = np.stack([m["x0"], 0.5 * m["x0"], 0.1 * m["x0"]])
    s = _solver32(m)
    s.chock_batch(X, k, 0.0, a)
    s.chock_batch(X, k, 0.0, a, warm=True)
    long = _solver32(m)
    long.chock_batch(X, 2 * k + 1, 0.0, a)
    for b in range(3):
        assert trace_rel_err(s.batch_error_cache[b], long.batch_error_cache[b][k + 1:]) <= TRACE_TOL
        assert trace_rel_err(s.batch_delta_error_cache[b], long.batch_delta_error_cache[b][k + 1:]) <= TRACE_TOL
        assert rel_err(s.batch_primal_flat(b), long.batch_primal_flat(b)) <= Z_TOL
        assert rel_err(s.batch_dual_flat(b), long.batch_dual_flat(b)) <= Z_TOL
    with pytest.raises(ValueError):
        s.chock_batch(X[:2], k, 0.0, a, warm=True)
