"""GPU: Anderson-accelerated closed-loop simulation of a batch (Solver.simulate_batch(accel=m),
raocp_cp_batch_mpc_aa, k_cpa + k_mpc_step_aa).

The central check is the replay of tests/test_gpu_mpc.py with the accelerated kernel: k_cpa is
bitwise invariant to batch size, position and chunking (tests/test_gpu_batch_accel.py) and a warm
chock_batch(accel=m) documents that it starts with an empty history, so step t of the resident run
must be bit-identical to chock_batch(states[:, t], accel=m) started from the replay's own previous
final iterate (warm) or from zero. The replay is fed the device's recorded states, so nothing
compounds and every comparison is array_equal; the per-step counts are compared with a NumPy count
of the replay's log. Every problem comes from the committed fixtures; B = 3, T = 3 unless a test
says otherwise. Section 8 repeats the replay with memories 1 and 8 and a cadence of 3, on a ternary
tree with dense weights and on the tree whose tables k_cpa<false> reads from HBM
(tests/branch_cases.py), and runs a simulation whose every solve is refused (accel_reg = inf): the
plain simulation bit for bit, with the fourth counter a closed form of the iteration count.
"""
import contextlib
import os

import numpy as np
import pytest

import accel_cases as ac
import accel_ref
import branch_cases as bc
import raocp.core as core
from raocp.core._native import RaocpError
from helpers import problem_from_golden

pytestmark = pytest.mark.gpu

FIXTURE = {"main": "main_trace", "c1n5": "traj_small"}
FIELDS = ("states", "inputs", "stage_costs", "status", "iterations", "errors", "accel_counts")


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
    """A fixture problem, its pinned alpha, three distinct initial states and scenario paths that
    cover every child of the root (built once)."""
    if name not in _PROB:
        z = golden(FIXTURE[name])
        r, tree, prob = problem_from_golden(z, name)
        x0 = np.asarray(r["x0"], dtype=float).reshape(-1)
        nc = len(tree.children_of(0))
        scen = np.array([[(b + t) % nc for t in range(3)] for b in range(3)], dtype=np.int64)
        assert set(scen.reshape(-1)) == set(range(nc))
        _PROB[name] = dict(prob=prob, x0=x0, alpha=float(z[f"{name}/cp_alpha"]), nc=nc,
                           X=np.stack([x0, 0.5 * x0, -0.3 * x0]), scen=scen)
    return _PROB[name]


def counts_of_log(log):
    """Proposals made, trials accepted, trials rejected, solves refused of one (rows, 12) log."""
    log = np.atleast_2d(log)
    return np.array([np.count_nonzero(log[:, 2] == 1), np.count_nonzero(log[:, 0] == 2),
                     np.count_nonzero(log[:, 0] == 3), np.count_nonzero(log[:, 2] == 2)])


class Run:
    """One resident run with what the solver reports about every instance's last solve."""

    def __init__(self, m, X, scen, K, tol, warm, raises=False, accel=5, **aa):
        s = core.Solver(problem_spec=m["prob"])
        kw = dict(scenarios=scen, max_iters=K, tol=tol, step_size=m["alpha"], warm=warm, accel=accel, **aa)
        if raises:
            with pytest.raises(ValueError) as ei:
                s.simulate_batch(X, scen.shape[1], **kw)
            self.message = str(ei.value)
            self.res = s.batch_simulation
        else:
            self.res = s.simulate_batch(X, scen.shape[1], **kw)
            assert self.res is s.batch_simulation
        B = X.shape[0]
        self.solver = s
        self.fin = [(s.batch_primal_flat(b), s.batch_dual_flat(b)) for b in range(B)]
        self.logs = list(s.batch_accel_log)
        self.first = s.batch_first_inputs()

    def of(self, q):
        """Everything about instance q, for the invariance checks."""
        return tuple(getattr(self.res, f)[q] for f in FIELDS) + (self.fin[q][0], self.fin[q][1], self.logs[q], self.first[q])


def _last_rows(solver, B):
    return np.stack([np.atleast_2d(solver.batch_error_cache[b])[-1] for b in range(B)])


def _rows(solver, B):
    return np.array([np.atleast_2d(solver.batch_error_cache[b]).shape[0] for b in range(B)])


def _assert_replay_bitwise(m, run, K, tol, warm, accel=5, **aa):
    """Every step of the resident run against a host-driven chock_batch(accel=m) from the device's
    recorded state; returns the replay's per-step logs."""
    res = run.res
    B, T = res.scenarios.shape
    assert res.accel_counts.shape == (B, T, 4) and np.issubdtype(res.accel_counts.dtype, np.integer)
    rep = core.Solver(problem_spec=m["prob"])
    logs = []
    for t in range(T):
        st = rep.chock_batch(res.states[:, t], max_iters=K, tol=tol, step_size=m["alpha"], warm=warm and t > 0,
                             accel=accel, **aa)
        assert np.array_equal(res.status[:, t], st), t
        assert np.array_equal(res.iterations[:, t], _rows(rep, B)), t
        assert np.array_equal(res.errors[:, t], _last_rows(rep, B)), t
        assert np.array_equal(res.inputs[:, t], rep.batch_first_inputs()), t
        want = np.stack([counts_of_log(rep.batch_accel_log[b]) for b in range(B)])
        assert np.array_equal(res.accel_counts[:, t], want), (t, res.accel_counts[:, t], want)
        for b in range(B):   # an empty history at the start of every step
            assert rep.batch_accel_log[b][0, 0] == 0 and rep.batch_accel_log[b][0, 1] == 0, (t, b)
        logs.append(list(rep.batch_accel_log))
    for b in range(B):
        assert np.array_equal(run.fin[b][0], rep.batch_primal_flat(b)), b
        assert np.array_equal(run.fin[b][1], rep.batch_dual_flat(b)), b
        assert np.array_equal(run.logs[b], rep.batch_accel_log[b]), b
    assert np.array_equal(run.first, rep.batch_first_inputs())
    # the follow-up calls describe the same last solve on both solvers
    ea, eb = run.solver.evaluate_batch(), rep.evaluate_batch()
    for f in ("cost", "epigraph", "box_violation", "dynamics_residual"):
        assert np.array_equal(getattr(ea, f), getattr(eb, f)), f
    return logs


# ---- 1. the feature is there

@pytest.mark.parametrize("name", ["main", "c1n5"])
def test_accel_counts_and_proposals_in_every_step(golden, name):
    m = _problem(golden, name)
    run = Run(m, m["X"], m["scen"], 30, 0.0, True)
    res = run.res
    assert isinstance(res, core.BatchSimulation)
    assert res.accel_counts.shape == (3, 3, 4)
    print(name, "accel_counts", res.accel_counts.tolist())
    assert np.all(res.accel_counts[:, :, 0] >= 1)          # a proposal in every step of every instance
    assert np.all(res.accel_counts >= 0) and np.all(res.iterations == 31) and np.all(res.status == 1)
    # every proposal has its trial: the iteration that stops a solve never makes one
    assert np.array_equal(res.accel_counts[:, :, 1] + res.accel_counts[:, :, 2], res.accel_counts[:, :, 0])
    for b in range(3):
        assert run.logs[b].shape == (31, 12)
        assert np.array_equal(res.accel_counts[b, -1], counts_of_log(run.logs[b]))


# ---- 2. the replay, bit for bit

CASES = [("main", 29), ("main", 30), ("main", 31), ("c1n5", 30)]


@pytest.mark.parametrize("warm", [True, False])
@pytest.mark.parametrize("name,K", CASES)
def test_replay_bitwise_to_max_iters(golden, name, K, warm):
    """tol = 0: every solve runs to max_iters, and with a proposal every iteration the last one
    is the trial of a proposal that was pending when the solve stopped. max_iters 29 / 30 / 31
    leave the final primal in rotation slots 0 / 1 / 2 and the final dual in slots 0 / 1 / 0."""
    m = _problem(golden, name)
    run = Run(m, m["X"], m["scen"], K, 0.0, warm)
    assert np.all(run.res.iterations == K + 1) and np.all(run.res.status == 1)
    logs = _assert_replay_bitwise(m, run, K, 0.0, warm)
    pend = [bool(logs[t][b][K - 1, 2] == 1) for t in range(3) for b in range(3)]
    print(name, K, warm, "a proposal pending at the stop:", pend)
    assert any(pend)


@pytest.mark.parametrize("warm", [True, False])
def test_replay_bitwise_with_per_instance_stopping(golden, warm):
    """A tolerance the instances meet at different iterations, chosen from the error traces of the
    host-driven solve of step 0."""
    m = _problem(golden, "main")
    K = 40
    probe = core.Solver(problem_spec=m["prob"])
    probe.chock_batch(m["X"], max_iters=K, tol=0.0, step_size=m["alpha"], accel=5)
    traces = [np.max(np.atleast_2d(probe.batch_error_cache[b]), axis=1) for b in range(3)]
    best = None
    for cand in sorted({float(v) for tr in traces for v in tr[3:K - 2]}, reverse=True):
        hits = [int(np.argmax(tr <= cand)) if np.any(tr <= cand) else K for tr in traces]
        key = (len({h for h in hits if h < K}), -max(hits))
        if best is None or key > best[0]:
            best = (key, cand, hits)
    (_, tol, hits) = best
    print("tol", tol, "first rows at or below it", hits)
    run = Run(m, m["X"], m["scen"], K, tol, warm)
    it0 = run.res.iterations[:, 0]
    print("iterations", run.res.iterations.tolist(), "status", run.res.status.tolist())
    assert len({int(v) for v in it0 if v < K + 1}) >= 2       # two instances stop at different k
    _assert_replay_bitwise(m, run, K, tol, warm)


# ---- 3. both trial outcomes

@pytest.mark.parametrize("name", ["main", "c1n5"])
def test_every_trial_rejected_restores_across_steps(golden, name):
    m = _problem(golden, name)
    run = Run(m, m["X"], m["scen"], 30, 0.0, True, accel_safeguard=0.0)
    c = run.res.accel_counts
    print(name, "accel_counts", c.tolist())
    assert np.all(c[:, :, 1] == 0) and np.all(c[:, :, 2] >= 1)
    _assert_replay_bitwise(m, run, 30, 0.0, True, accel_safeguard=0.0)


@pytest.mark.parametrize("name", ["main", "c1n5"])
def test_every_trial_accepted(golden, name):
    m = _problem(golden, name)
    run = Run(m, m["X"], m["scen"], 30, 0.0, True, accel_safeguard=1e300)
    c = run.res.accel_counts
    print(name, "accel_counts", c.tolist())
    assert np.all(c[:, :, 2] == 0) and np.all(c[:, :, 1] >= 1)


# ---- 4. the history does not leak across steps

def test_history_does_not_leak_across_steps(golden):
    """T = 2, warm: the second step equals a fresh chock_batch(accel=5, warm=True) from the first
    step's iterate (the replay at t = 1). The device's own log of the last step of a run of 1, 2
    and 3 steps starts with an empty history, and the shorter runs are prefixes of the longer."""
    m = _problem(golden, "main")
    runs = {T: Run(m, m["X"], m["scen"][:, :T], 30, 0.0, True) for T in (1, 2, 3)}
    _assert_replay_bitwise(m, runs[2], 30, 0.0, True)
    for T, run in runs.items():
        for b in range(3):
            log = run.logs[b]
            assert log[0, 0] == 0 and log[0, 1] == 0 and log[0, 2] == 0, (T, b, log[0])
            assert log[1, 1] == 1 and log[1, 2] == 1, (T, b, log[1])    # one column, the first proposal
        for f in FIELDS:
            got, ref = getattr(run.res, f), getattr(runs[3].res, f)
            n = T + 1 if f == "states" else T
            assert np.array_equal(got, ref[:, :n]), (T, f)


# ---- 5. chunk, batch size and position

def _run_at(m, B, pos, chunk, K=20, T=3):
    rng = np.random.default_rng(5)
    X = m["x0"][None, :] * (0.05 + rng.random((B, 1))) + 0.01 * rng.standard_normal((B, m["x0"].size))
    scen = rng.integers(0, m["nc"], size=(B, T))
    for q in pos:
        X[q] = m["x0"]
        scen[q] = [t % m["nc"] for t in range(T)]
    with env(RAOCP_BATCH_CHUNK=chunk):
        run = Run(m, X, scen, K, 0.0, True)
    return [run.of(q) for q in pos]


def test_chunk_batch_and_position_invariance_bitwise(golden):
    m = _problem(golden, "main")
    ref = _run_at(m, 1, [0], 256)[0]
    assert np.all(ref[6][:, 0] >= 5)     # proposals in every step, so chunk 1 splits them from their trials
    for chunk in (1, 256):
        got = _run_at(m, 1, [0], chunk) + _run_at(m, 5, [0, 4], chunk)
        for g in got:
            for a, b in zip(g, ref):
                assert np.array_equal(a, b), chunk


# ---- 6. NaN isolation

def test_nan_isolation_and_freezing(golden):
    m = _problem(golden, "main")
    x0 = m["x0"]
    X = np.stack([x0, 0.5 * x0, 0.3 * x0, 0.1 * x0])
    scen = np.array([[0, 1, 2], [1, 2, 0], [2, 0, 1], [1, 1, 0]])
    keep = [0, 1, 3]
    good = Run(m, X[keep], scen[keep], 30, 0.0, True)       # a run without the poisoned instance
    Xn = X.copy()
    Xn[2, 0] = np.nan
    bad = Run(m, Xn, scen, 30, 0.0, True, raises=True)
    assert "instances [2]" in bad.message and "steps [0]" in bad.message
    r = bad.res
    assert np.all(r.status[2] == 2) and r.iterations[2, 0] > 0 and np.all(r.iterations[2, 1:] == 0)
    assert np.all(np.isnan(r.states[2, 1:])) and np.all(np.isnan(r.inputs[2])) and np.all(np.isnan(r.stage_costs[2]))
    assert np.all(np.isnan(r.errors[2, 1:]))
    assert np.all(r.accel_counts[2, 1:] == 0)
    # the step that froze it has the counts of that solve, and the log is still that solve's
    assert bad.logs[2].shape == (int(r.iterations[2, 0]), 12)
    assert np.array_equal(r.accel_counts[2, 0], counts_of_log(bad.logs[2]))
    for q, b in enumerate(keep):
        for x, y in zip(bad.of(b), good.of(q)):
            assert np.array_equal(x, y), b


# ---- 7. accel = 0 is the call as it was; refusals

def test_accel_zero_is_the_plain_simulation_and_refusals(golden):
    m = _problem(golden, "main")
    kw = dict(scenarios=m["scen"], max_iters=30, tol=0.0, step_size=m["alpha"])
    a = core.Solver(problem_spec=m["prob"])
    b = core.Solver(problem_spec=m["prob"])
    ra = a.simulate_batch(m["X"], 3, **kw)
    rb = b.simulate_batch(m["X"], 3, accel=0, **kw)
    assert ra.accel_counts is None and rb.accel_counts is None and b.batch_accel_log == []
    for f in FIELDS[:-1] + ("scenarios",):
        assert np.array_equal(getattr(ra, f), getattr(rb, f)), f
    for q in range(3):
        assert np.array_equal(a.batch_primal_flat(q), b.batch_primal_flat(q))
        assert np.array_equal(a.batch_dual_flat(q), b.batch_dual_flat(q))
    assert np.array_equal(a.batch_first_inputs(), b.batch_first_inputs())
    nat = a.cache.native
    assert nat.kernel_info(14) == "k_mpc_step"
    assert nat.kernel_info(20) == "k_mpc_step_aa"
    assert nat.kernel_info(13) in ("k_cpb<true>", "k_cpb<false>") and nat.kernel_info(19) in ("k_cpa<true>", "k_cpa<false>")
    # the accelerated run differs from the plain one (it is not the same call under another name)
    rc = Run(m, m["X"], m["scen"], 30, 0.0, True).res
    assert not np.array_equal(rc.errors, ra.errors)
    # the C entry point's own checks: those of the plain call, then those of the accelerated solve
    nx = m["x0"].size
    sc = np.zeros((2, 2), dtype=np.int32)
    for args, accel in (((np.zeros((2, nx)), sc, 1, 0.0, m["alpha"]), (9, 1, 1e-10, 1.0)),
                        ((np.zeros((2, nx)), sc, 1, 0.0, m["alpha"]), (0, 1, 1e-10, 1.0)),
                        ((np.zeros((2, nx)), sc, 1, 0.0, m["alpha"]), (5, 0, 1e-10, 1.0)),
                        ((np.zeros((2, nx)), sc, 1, 0.0, m["alpha"]), (5, 1, -1.0, 1.0)),
                        ((np.zeros((2, nx)), sc, 1, 0.0, m["alpha"]), (5, 1, 1e-10, -1.0)),
                        ((np.zeros((2, nx)), sc, -1, 0.0, m["alpha"]), (5, 1, 1e-10, 1.0)),
                        ((np.zeros((2, nx)), np.zeros((2, 0), dtype=np.int32), 1, 0.0, m["alpha"]), (5, 1, 1e-10, 1.0)),
                        ((np.zeros((2, nx)), sc + m["nc"], 1, 0.0, m["alpha"]), (5, 1, 1e-10, 1.0))):
        with pytest.raises(RaocpError):
            nat.cp_batch_mpc(*args, accel=accel)
    # a float32 solver and a context the batch kernel does not cover: no accelerated form
    s32 = core.Solver(problem_spec=m["prob"], dtype="float32")
    assert s32.cache.native.kernel_info(20) == ""
    with pytest.raises(ValueError):
        s32.simulate_batch(m["X"], 3, accel=5, **kw)
    with pytest.raises(RaocpError):
        s32.cache.native.cp_batch_mpc(m["X"], m["scen"], 30, 0.0, m["alpha"], accel=(5, 1, 1e-10, 1.0))
    with env(RAOCP_CPB=0):
        assert nat.kernel_info(20) == "" and nat.kernel_info(14) == ""
        with pytest.raises(ValueError):
            a.simulate_batch(m["X"], 3, accel=5, **kw)
    assert nat.kernel_info(20) == "k_mpc_step_aa"
    for bad in (9, -1, 2.5):
        with pytest.raises(ValueError):
            a.simulate_batch(m["X"], 3, accel=bad, **kw)
    with pytest.raises(ValueError):
        a.simulate_batch(m["X"], 3, accel=5, accel_every=0, **kw)
    # nothing of the refused calls replaced the last result
    assert a.batch_simulation is ra


# ---- 8. other memories, cadences and trees; every solve refused; a context without the kernels

def _tree_problem(tree):
    """_problem for a tree of tests/branch_cases.py: its alpha (pinned or the oracle's own), x0, 0.5 x0
    and -0.3 x0, scenario paths over the root's children the way _problem builds them."""
    key = ("tree", tree)   # _problem's entries (by fixture name) hold no oracle
    if key not in _PROB:
        r, prob, op, alpha = bc.problem(tree)
        x0 = np.asarray(r["x0"], dtype=float).reshape(-1)
        nc = len(prob.tree.children_of(0))
        scen = np.array([[(b + t) % nc for t in range(3)] for b in range(3)], dtype=np.int64)
        assert set(scen.reshape(-1)) == set(range(nc))
        _PROB[key] = dict(prob=prob, orc=op, x0=x0, alpha=alpha, nc=nc, X=np.stack([x0, 0.5 * x0, -0.3 * x0]), scen=scen)
    return _PROB[key]


GRID = [("main", 1, 1), ("main", 8, 1), ("main", 3, 3), ("s5x3", 8, 1), ("m7x32", 8, 1)]


@pytest.mark.parametrize("warm", [True, False])
@pytest.mark.parametrize("tree,accel,every", GRID)
def test_replay_bitwise_over_memories_cadences_and_trees(tree, accel, every, warm):
    """The replay of section 2 with the degenerate ring (1), the full one (8: with K = 30 it fills
    and wraps in every step) and a cadence of 3, and with memory 8 on a ternary tree with dense
    weights per mode and on the 7-mode tree whose tables k_cpa<false> reads from HBM."""
    m = _tree_problem(tree)
    run = Run(m, m["X"], m["scen"], 30, 0.0, warm, accel=accel, accel_every=every)
    nat = run.solver.cache.native
    assert nat.kernel_info(19) == bc.CPA_KERNEL[tree] and nat.kernel_info(20) == "k_mpc_step_aa"
    assert np.all(run.res.iterations == 31) and np.all(run.res.status == 1)
    logs = _assert_replay_bitwise(m, run, 30, 0.0, warm, accel=accel, accel_every=every)
    c = run.res.accel_counts
    print(tree, accel, every, warm, "accel_counts", c.tolist())
    assert np.all(c[:, :, 0] >= 1) and np.all(c[:, :, 3] == 0)      # proposals in every step of every instance
    for b in range(3):   # step 0 is the cold solve from X: the ring fills (tests/test_accel_host.py, the free model)
        assert logs[0][b][:, 1].max() == accel and c[b, 0, 0] >= 5, (b, logs[0][b][:, :3].astype(int).tolist())
    if every > 1:        # a proposal only where (k + 1) % every == 0
        off = [k for k in range(31) if (k + 1) % every]
        assert not any(logs[t][b][off, 2].any() for t in range(3) for b in range(3))


@pytest.mark.parametrize("warm", [True, False])
@pytest.mark.parametrize("tree", ["main", "s5x3", "m7x32"])
def test_every_solve_refused_is_the_plain_simulation_bitwise(tree, warm):
    """accel_reg = inf: aa_solve refuses every system at its first pivot, so every step is the plain
    step and the fourth counter is the only one that moves. With a trial every iteration a solve
    of n iterations refuses at every odd k below its stopping record: (n - 1) // 2 times
    (accel_cases.refusals_of), whatever the trajectory; the free model says the same."""
    m = _tree_problem(tree)
    run = Run(m, m["X"], m["scen"], 30, 0.0, warm, accel=5, accel_reg=float("inf"))
    plain = core.Solver(problem_spec=m["prob"])
    rp = plain.simulate_batch(m["X"], 3, scenarios=m["scen"], max_iters=30, tol=0.0, step_size=m["alpha"], warm=warm)
    for f in FIELDS[:-1] + ("scenarios",):
        assert np.array_equal(getattr(run.res, f), getattr(rp, f)), f
    for b in range(3):
        assert np.array_equal(run.fin[b][0], plain.batch_primal_flat(b)) and np.array_equal(run.fin[b][1], plain.batch_dual_flat(b))
    assert np.array_equal(run.first, plain.batch_first_inputs())
    c = run.res.accel_counts
    print(tree, warm, "accel_counts", c.tolist())
    assert np.all(c[:, :, 0:3] == 0)
    assert np.all(run.res.iterations == 31) and ac.refusals_of(31, 1) == 15
    assert np.array_equal(c[:, :, 3], (run.res.iterations - 1) // 2) and np.all(c[:, :, 3] == 15)
    ref = accel_ref.run(m["orc"], m["X"][0], m["alpha"], 30, 0.0, m=5, reg=float("inf"))
    assert np.array_equal(counts_of_log(ref.log), [0, 0, 0, 15])
    for b in range(3):   # the last step's log: the model's records but for |r|_2, which no decision reads here
        assert np.array_equal(run.logs[b][:, :3], ref.log[:, :3]) and not run.logs[b][:, 4:].any()
        assert np.array_equal(c[b, -1], counts_of_log(run.logs[b]))


def test_a_context_the_batch_kernel_does_not_cover_has_no_accelerated_form():
    """s6x18: nu = 18 is beyond the 16 inputs k_cpb covers, so the plain calls fall back to the
    sequential solves and the accelerated ones, which have no such form, refuse before any launch."""
    r, prob, op, alpha = bc.problem("s6x18")
    s = core.Solver(problem_spec=prob)
    nat = s.cache.native
    assert nat.kernel_info(19) == nat.kernel_info(20) == "" and nat.kernel_info(13) == ""
    x0 = np.asarray(r["x0"], dtype=float).reshape(-1)
    X = np.stack([x0, 0.5 * x0])
    scen = np.zeros((2, 2), dtype=np.int64)
    with pytest.raises(ValueError):
        s.chock_batch(X, 5, 0.0, alpha, accel=5)
    with pytest.raises(ValueError):
        s.simulate_batch(X, 2, scenarios=scen, max_iters=5, tol=0.0, step_size=alpha, accel=5)
    with pytest.raises(RaocpError):
        nat.cp_batch_run(X, 5, 0.0, alpha, accel=(5, 1, 1e-10, 1.0))
    with pytest.raises(RaocpError):
        nat.cp_batch_mpc(X, scen, 5, 0.0, alpha, accel=(5, 1, 1e-10, 1.0))
    assert s.batch_error_cache == [] and s.batch_simulation is None
