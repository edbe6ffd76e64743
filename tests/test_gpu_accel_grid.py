"""GPU: k_cpa (Solver.chock_batch(accel=m), raocp_cp_batch_run_aa) over memories, cadences,
regularisations, safeguards, both forms of the kernel, general shapes, caller-supplied starts and
reused solvers, against tests/accel_ref.py, the NumPy model over OracleProblem.cp_iteration.

The grid (tests/accel_cases.py), (m, every, reg, safeguard):
    m1 (1, 1, 1e-10, 1)   m2 (2, 1, 1e-10, 1)   m8 (8, 1, 1e-10, 1)   m3e3 (3, 3, 1e-10, 1)
    m5e2r0 (5, 2, 0, 1)   m4r1e-2 (4, 1, 1e-2, 1)   m5s.5 (5, 1, 1e-10, 0.5)
The trees (tests/branch_cases.problem) and the form of the kernel each reaches (kernel_info(19),
bc.CPA_KERNEL; asserted in every case):
    main         golden, 3 / 2, 43 nodes                                     k_cpa<true>   whole grid
    s5x3         ternary, dense weights per mode, uneven boxes, 5 / 3         k_cpa<true>   whole grid
    m7x32        7 modes, 32 / 12, 75 KB of tables read from HBM              k_cpa<false>  whole grid
    s1x1         1 / 1                                                        k_cpa<true>   m1 m8 m3e3
    s17x5        ternary, 17 / 5                                              k_cpa<true>   m1 m8 m3e3
    s16x16       nu at the kernel's limit                                     k_cpa<true>   m1 m8 m3e3
    m7x32-dense  m7x32 with dense tables per mode and one-sided bounds        k_cpa<false>  m1 m8 m3e3
    g53          27 nodes, 1 / 2 / 3 children per node, 5 / 3                 k_cpa<true>   m1 m8 m3e3
K = 40, tol = 0, B = 3 from x0, 0.5 x0, -0.3 x0 (m7x32-dense: 0.75 x0, accel_cases.SCALES_OF); alpha
is the fixtures' pinned one or the oracle's own.

Bounds, and where each comes from.
  * Against the replay of the device's log (accel_ref.run(log=)): 1e-8 per history entry and 1e-10
    of the largest entry on z and eta, the bounds of tests/test_gpu_drc.py and
    tests/test_gpu_batch_accel.py against the same oracle; log columns 0..2 equal; |r|_2 within
    1e-8 max(1, .); every trial decision equal to the model's inequality unless its two sides are
    within 1e-8 relative; the backward error of every gamma on the model's own system within
    1e-10 (|Gbar|_F |gamma|_2 + |b|_2) (tests/test_gpu_batch_accel.py derives it: summation order
    and Cholesky rounding are of order eps (P + D) m).
  * gamma is exactly zero beyond j and wherever no proposal was made (the kernel stores zeros).
  * The coverage conditions of accel_cases.coverage_violations hold on the device's log, so no case
    passes without a full ring overwritten after the wrap, columns pushed off the cadence, or the
    rejections its options are there for; tests/test_accel_host.py pins that the free model alone
    meets them.
  * accel_reg = inf: aa_solve refuses at the first pivot (the shift is inf, or NaN on a zero
    trace), on the device as in the model, whatever the rounding. Such a solve is the plain solve:
    histories, iterates and first inputs are bit for bit those of chock_batch without acceleration,
    and the log's code, j, prop and gamma columns equal the free model's. The |r|_2 column is a
    floating-point norm the two compute by different arithmetic (a wave tree of fma sums against
    NumPy on the oracle's iterate), so it is held to the project's 1e-8 max(1, .) like everywhere
    else rather than to equality.
  * One solver reused over batches of other B, m and K, and a warm batch: everything equal, bit
    for bit, to a fresh solver that runs only that step (k_cpa is invariant to what ran before).
"""
import numpy as np
import pytest

import accel_cases as ac
import accel_ref
import branch_cases as bc
import raocp.core as core
from raocp.core._native import RaocpError

pytestmark = pytest.mark.gpu

INF = float("inf")


def _results(s, b):
    return (np.atleast_2d(s.batch_error_cache[b]), np.atleast_2d(s.batch_delta_error_cache[b]),
            s.batch_primal_flat(b), s.batch_dual_flat(b))


def _assert_replay(tag, op, x0, alpha, K, opts, log, err, derr, z, eta, p0=None, d0=None):
    """The device's solve against the model's replay of its log, with the project's bounds."""
    m, every, reg, sg = opts
    ref = accel_ref.run(op, x0, alpha, K, 0.0, m=m, every=every, reg=reg, safeguard=sg, log=log, p0=p0, d0=d0)
    assert err.shape == ref.err.shape and log.shape == ref.log.shape == (K + 1, 12)
    d_err = float(np.max(np.abs(err - ref.err)))
    d_derr = float(np.max(np.abs(derr - ref.derr)))
    d_z = float(np.max(np.abs(z - ref.z))) / float(np.max(np.abs(ref.z)))
    d_eta = float(np.max(np.abs(eta - ref.eta))) / max(float(np.max(np.abs(ref.eta))), 1e-300)
    d_rn = float(np.max(np.abs(log[:, 3] - ref.log[:, 3]) / np.maximum(1.0, ref.log[:, 3])))
    worst = 0.0
    for k, Gb, bb, gam in ref.systems:
        res = float(np.linalg.norm(Gb @ gam - bb))
        bound = 1e-10 * (float(np.linalg.norm(Gb)) * float(np.linalg.norm(gam)) + float(np.linalg.norm(bb)))
        worst = max(worst, res / bound if bound > 0 else (0.0 if res == 0 else np.inf))
    codes = np.bincount(log[:, 0].astype(int), minlength=5)
    print(f"accel-grid {tag}: codes {codes.tolist()} err {d_err:.2e} derr {d_derr:.2e} z {d_z:.2e} eta {d_eta:.2e} "
          f"|r| {d_rn:.2e} gamma residual / bound {worst:.2e} over {len(ref.systems)}")
    assert np.isfinite(z).all() and np.isfinite(eta).all()
    assert np.array_equal(log[:, :3], ref.log[:, :3]), tag
    assert d_err <= 1e-8 and d_derr <= 1e-8, tag
    assert d_z <= 1e-10 and d_eta <= 1e-10, tag
    assert d_rn <= 1e-8, tag
    for k, lhs, rhs, code in ref.trials:
        if abs(lhs - rhs) > 1e-8 * max(lhs, rhs):
            assert code == (2 if lhs <= rhs else 3), (tag, k, lhs, rhs, code)
    assert worst <= 1.0, tag
    assert ac.gamma_violations(log) == [], tag
    return ref


# ---- 1. replay against the oracle over the option grid

@pytest.mark.parametrize("tree,opt", ac.CASES, ids=[f"{t}-{o}" for t, o in ac.CASES])
def test_replay_against_the_oracle_over_the_grid(tree, opt):
    r, prob, op, alpha = bc.problem(tree)
    m, every, reg, sg = ac.OPTS[opt]
    X = ac.states(tree)
    s = core.Solver(problem_spec=prob)
    assert s.cache.native.kernel_info(19) == bc.CPA_KERNEL[tree]
    st = s.chock_batch(X, max_iters=ac.K, tol=0.0, step_size=alpha, accel=m, accel_every=every, accel_reg=reg,
                       accel_safeguard=sg)
    assert np.array_equal(st, [1, 1, 1])
    for b in range(3):
        log = s.batch_accel_log[b]
        assert ac.coverage_violations(log, opt) == [], (tree, opt, b, log[:, :3].astype(int).tolist())
        _assert_replay(f"{tree} {opt} [{b}]", op, X[b], alpha, ac.K, ac.OPTS[opt], log, *_results(s, b))


# ---- 2. every solve refused is the plain solve, bit for bit

_PLAIN = {}


def _plain(tree, K):
    """The plain batch of the tree's three states: (histories and iterates per instance, first
    inputs), computed once and read-only."""
    if (tree, K) not in _PLAIN:
        r, prob, op, alpha = bc.problem(tree)
        s = core.Solver(problem_spec=prob)
        s.chock_batch(ac.states(tree), max_iters=K, tol=0.0, step_size=alpha)
        assert s.batch_accel_log == []
        out = [_results(s, b) for b in range(3)], s.batch_first_inputs()
        for a in [x for res in out[0] for x in res] + [out[1]]:
            a.setflags(write=False)
        _PLAIN[(tree, K)] = out
    return _PLAIN[(tree, K)]


@pytest.mark.parametrize("K", [30, 31])
@pytest.mark.parametrize("every", [1, 3])
@pytest.mark.parametrize("m", [1, 5, 8])
@pytest.mark.parametrize("tree", ac.FULL_TREES)
def test_every_solve_refused_is_the_plain_solve_bitwise(tree, m, every, K):
    """K = 30 and 31: with every = 1 the refusals fall on odd k, so the iteration that stops the
    solve of K = 31 is one that would have solved (with every = 3, k = 2 mod 3: neither K)."""
    r, prob, op, alpha = bc.problem(tree)
    X = ac.states(tree)
    s = core.Solver(problem_spec=prob)
    assert s.cache.native.kernel_info(19) == bc.CPA_KERNEL[tree]
    st = s.chock_batch(X, max_iters=K, tol=0.0, step_size=alpha, accel=m, accel_every=every, accel_reg=INF)
    plain, first = _plain(tree, K)
    assert np.array_equal(st, [1, 1, 1]) and np.array_equal(s.batch_first_inputs(), first)
    for b in range(3):
        for x, y in zip(_results(s, b), plain[b]):
            assert np.array_equal(x, y), (tree, m, every, K, b)
        log = s.batch_accel_log[b]
        ref = accel_ref.run(op, X[b], alpha, K, 0.0, m=m, every=every, reg=INF)
        code, j, prop = (log[:, q].astype(int) for q in range(3))
        assert log.shape == ref.log.shape == (K + 1, 12)
        assert np.array_equal(log[:, :3], ref.log[:, :3]), (log[:, :3].astype(int).tolist(), ref.log[:, :3].astype(int).tolist())
        assert np.array_equal(log[:, 4:], ref.log[:, 4:]) and not log[:, 4:].any()
        d_rn = float(np.max(np.abs(log[:, 3] - ref.log[:, 3]) / np.maximum(1.0, ref.log[:, 3])))
        assert d_rn <= 1e-8, d_rn
        # what the model's log says, stated: only plain and refused records, code 4 with prop 2, a
        # cleared history (the previous pair included) after each, the stopping record plain
        assert set(code) == {0, 4} and np.array_equal(code == 4, prop == 2) and code[-1] == 0 and j[-1] == 0
        hit = np.flatnonzero(code == 4)
        assert hit.size == ac.refusals_of(K + 1, every) >= 9
        assert np.all(j[hit] == min(m, 1 if every == 1 else every - 1))
        assert np.all(j[hit + 1] == 0) and np.all(code[hit + 1] == 0)
        assert np.all(j[hit[hit + 2 <= K - 1] + 2] == 1)      # one held pair later the first column again
        if every == 1:   # K = 30: k = 29 is refused and k = 30 stops on the held pair; K = 31: k = 31 would have solved
            assert (K - 1 in hit) == (K % 2 == 0)


# ---- 3. crafted and caller-supplied starts

CRAFT_SCALES = (1.0, 0.5, 0.1)


def _crafted(tree):
    r, prob, op, alpha = bc.problem(tree)
    seeds = bc.BATCH_SEEDS[tree]
    X = np.stack([sc * np.asarray(r["x0"], dtype=float).reshape(-1) for sc in CRAFT_SCALES])
    Z0 = np.stack([bc.start(tree, 0, sd)[0] for sd in seeds])
    E0 = np.stack([bc.start(tree, 0, sd)[1] for sd in seeds])
    return X, Z0, E0


@pytest.mark.parametrize("tree", bc.BATCH_TREES)
def test_crafted_starts_with_every_solve_refused_are_the_plain_batch_bitwise(tree):
    """The starts of test_gpu_branches.test_batch_kernel_matches_oracle_from_crafted_starts (every
    branch of the dual step in iteration 1; tests/test_branch_census.py) through k_cpa's copy of the
    iteration, at that test's own ITERS."""
    r, prob, op, alpha = bc.problem(tree)
    X, Z0, E0 = _crafted(tree)
    nat = core.Cache(prob).native
    assert nat.kernel_info(19) == bc.BATCH_KERNEL[tree][0].replace("k_cpb", "k_cpa")
    for K in bc.ITERS:
        st, errs, derrs = nat.cp_batch_run(X, K, 0.0, alpha, Z0, E0)
        want = [(errs[b], derrs[b]) + nat.cp_batch_get(b) for b in range(3)]
        first = nat.cp_batch_first_inputs()
        for m in (1, 5, 8):
            st_a, errs_a, derrs_a = nat.cp_batch_run(X, K, 0.0, alpha, Z0, E0, accel=(m, 1, INF, 1.0))
            assert np.array_equal(st, st_a) and np.array_equal(first, nat.cp_batch_first_inputs())
            for b in range(3):
                got = (errs_a[b], derrs_a[b]) + nat.cp_batch_get(b)
                for x, y in zip(got, want[b]):
                    assert x.shape == y.shape and np.array_equal(x, y), (tree, K, m, b)
                log = nat.cp_batch_accel_log(b)
                assert log.shape == (K + 1, 12) and not log[:, 4:].any()
                assert log[:, :3].tolist() == ([[0, 0, 0]] if K == 0 else [[0, 0, 0], [4, 1, 2], [0, 0, 0]])


@pytest.mark.parametrize("tree", ["main", "m7x32"])
def test_crafted_starts_replay_against_the_oracle(tree):
    """accel = 5 with the default options from the crafted starts, K = 20 (the ring of 5 fills and
    wraps within 12): the replay's bounds, and a supplied start begins with an empty history."""
    r, prob, op, alpha = bc.problem(tree)
    X, Z0, E0 = _crafted(tree)
    K, opts = 20, (5, 1, 1e-10, 1.0)
    nat = core.Cache(prob).native
    assert nat.kernel_info(19) == bc.CPA_KERNEL[tree]
    st, errs, derrs = nat.cp_batch_run(X, K, 0.0, alpha, Z0, E0, accel=opts)
    for b in range(3):
        log = nat.cp_batch_accel_log(b)
        assert log[0, :3].tolist() == [0, 0, 0] and np.count_nonzero(log[:, 2] == 1) >= 5, log[:, :3].astype(int).tolist()
        z, eta = nat.cp_batch_get(b)
        _assert_replay(f"{tree} crafted [{b}]", op, X[b], alpha, K, opts, log, errs[b], derrs[b], z, eta, p0=Z0[b], d0=E0[b])


# ---- 4. reuse of one solver

STEPS = [dict(B=3, K=40, accel=8), dict(B=3, K=10, accel=2), dict(B=3, K=40, accel=0), dict(B=5, K=40, accel=8),
         dict(B=5, K=12, accel=8, warm=True)]


def _step(s, X, alpha, B, K, accel, warm=False):
    st = s.chock_batch(X[:B], max_iters=K, tol=0.0, step_size=alpha, warm=warm, accel=accel)
    ev = s.evaluate_batch()
    out = [st, s.batch_first_inputs(), ev.cost, ev.epigraph, ev.box_violation, ev.dynamics_residual]
    for b in range(B):
        out += list(_results(s, b))
    assert len(s.batch_accel_log) == (B if accel else 0)
    for log in s.batch_accel_log:
        assert log.shape == (K + 1, 12)
        out.append(log)
    return out


@pytest.mark.parametrize("tree", ["main", "m7x32"])
def test_one_solver_reused_equals_fresh_solvers_bitwise(tree):
    """batch_ensure / batch_ensure_aa keep the slabs and the log over steps 1 -> 2 -> 3 (same B, fewer
    rows; m 8 -> 2 reallocates the acceleration's slab) and reallocate everything at step 4 (B 3 -> 5);
    the log of step 2 is laid out by its own 11 rows in a buffer of 41."""
    r, prob, op, alpha = bc.problem(tree)
    x0 = np.asarray(r["x0"], dtype=float).reshape(-1)
    X = np.stack([sc * x0 for sc in (1.0, 0.5, -0.3, 0.8, -0.6)])
    s = core.Solver(problem_spec=prob)
    for n, step in enumerate(STEPS):
        got = _step(s, X, alpha, **step)
        fresh = core.Solver(problem_spec=prob)
        if step.get("warm"):
            _step(fresh, X, alpha, **STEPS[n - 1])
        want = _step(fresh, X, alpha, **step)
        assert len(got) == len(want)
        for q, (x, y) in enumerate(zip(got, want)):
            assert x.shape == y.shape and np.array_equal(x, y), (tree, n, q)
        if not step["accel"]:
            assert s.batch_accel_log == []
            with pytest.raises(RaocpError, match="error -5"):
                s.cache.native.cp_batch_accel_log(0)
        elif step.get("warm"):
            assert all(log[0, :3].tolist() == [0, 0, 0] for log in s.batch_accel_log)
