"""GPU: the cone and box branches of the dual step in every CP kernel family.

The suite's cold-started trajectories never leave the scaling branch of the second-order-cone
projection on the nx = 20 / nu = 8 trees and barely touch the boxes ("Branch coverage
of the dual step"), so each family here runs one and three CP iterations from a crafted warm
start (tests/branch_cases.py) whose first iteration takes the identity, zero and scaling
branches on a third of the cones each, every box branch and both signs under the eta1 / eta2
clamps, all clear of the comparisons' edges (tests/test_branch_census.py proves that with the
oracle alone). Every case asserts the kernel_info string of its family, so a silent fallback to
another kernel fails the test.

Bounds are the suite's own against the oracle: fp64 1e-10 on the iterate and 1e-8 per residual
trace entry (BASELINE.json north_star), fp32 2e-4 and 2e-3 (test_gpu_cp5.py); the iterate is
compared per segment (helpers.segment_rel_err), each against its own largest entry, so the
+-alpha T offsets in eta6 / eta13 cannot hide an error elsewhere. They were set for 20 to 30
iterations, hence loose for 1 to 3; a wrong branch is an O(1) error in its segment. The largest
errors seen on an MI355X are recorded in profiles/r12_branches/README.md.
"""
import contextlib
import os

import numpy as np
import pytest

import raocp.core as core
import branch_cases as bc
from helpers import segment_rel_err, trace_rel_err

pytestmark = pytest.mark.gpu

TOL = {"float64": (1e-10, 1e-8), "float32": (2e-4, 2e-3)}  # iterate per segment, per trace entry


@contextlib.contextmanager
def _env(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _seg_max(got, ref, op, kind):
    return max(segment_rel_err(got, ref, op, kind).values())


_RUNS = {}


def _family_runs(case):
    """{(rot, K): (status, err, derr, z, eta)} of a family's context from the crafted start(s) of
    its tree: a fresh context, created as the family's own tests select it; run once, shared
    by the oracle test and the agreement test."""
    if case not in _RUNS:
        _, tree, env, dtype, info = bc.FAMILY[case]
        r, prob, op, alpha = bc.problem(tree)
        with _env(env):
            cache = core.Cache(prob, dtype=dtype)
        for which, how, text in info:
            got = cache.native.kernel_info(which)
            assert got == text if how == "eq" else got.startswith(text), (case, which, got, text)
        runs = {}
        for rot in range(bc.rotations(tree)):
            p0, d0, _, _ = bc.start(tree, rot, bc.seed_of(tree), dtype == "float32")
            for K in bc.ITERS:
                cache.set_primal_flat(p0)
                cache.set_dual_flat(d0)
                st, err, derr = cache.native.cp_run(r["x0"], K, 0.0, alpha, warm=True)
                runs[(rot, K)] = (st, err, derr, cache.get_primal_flat(), cache.get_dual_flat())
        _RUNS[case] = runs
    return _RUNS[case]


@pytest.mark.parametrize("case", [c[0] for c in bc.FAMILIES])
def test_family_matches_oracle_from_crafted_start(case):
    _, tree, env, dtype, info = bc.FAMILY[case]
    r, prob, op, alpha = bc.problem(tree)
    tol_z, tol_t = TOL[dtype]
    worst = np.zeros(4)
    for (rot, K), (st, err, derr, z, e) in _family_runs(case).items():
        st_o, err_o, derr_o, z_o, e_o = bc.reference(tree, K, rot, bc.seed_of(tree), dtype == "float32")
        assert st == st_o == 1 and err.shape == err_o.shape == (K + 1, 3) and derr.shape == derr_o.shape
        got = np.array([_seg_max(z, z_o, op, "primal"), _seg_max(e, e_o, op, "dual"), trace_rel_err(err, err_o), trace_rel_err(derr, derr_o)])
        worst = np.fmax(worst, np.where(np.isnan(got), np.inf, got))
        print(f"branches {case} rot {rot} K {K}: primal {got[0]:.2e} dual {got[1]:.2e} traces {got[2]:.2e} / {got[3]:.2e}")
        assert np.isfinite(z).all() and np.isfinite(e).all()
        assert got[0] <= tol_z and got[1] <= tol_z, (case, rot, K, segment_rel_err(z, z_o, op, "primal"), segment_rel_err(e, e_o, op, "dual"))
        assert got[2] <= tol_t and got[3] <= tol_t, (case, rot, K, got)
    print(f"branches-max {case}: primal {worst[0]:.2e} dual {worst[1]:.2e} traces {worst[2]:.2e} / {worst[3]:.2e}")


@pytest.mark.parametrize("a,b,tol", bc.AGREE, ids=[f"{a}~{b}" for a, b, _ in bc.AGREE])
def test_kernels_sharing_arithmetic_agree_on_crafted_start(a, b, tol):
    """Kernels that claim one arithmetic (k_drc, k_cp6, k_cp4, k_cp3; k_cp5 and k_cp3: 1e-12; the
    two-launch MFMA kernels and the fused ones: 1e-10) agree with each other on the crafted
    start, per segment and per trace entry, within the bound the suite holds them to."""
    assert bc.FAMILY[a][1] == bc.FAMILY[b][1]
    op = bc.problem(bc.FAMILY[a][1])[2]
    ra, rb = _family_runs(a), _family_runs(b)
    assert ra.keys() == rb.keys()
    for key in ra:
        (sa, ea, da, za, ya), (sb, eb, db, zb, yb) = ra[key], rb[key]
        got = (_seg_max(za, zb, op, "primal"), _seg_max(ya, yb, op, "dual"), trace_rel_err(ea, eb), trace_rel_err(da, db))
        print(f"branches-agree {a} ~ {b} {key}: primal {got[0]:.2e} dual {got[1]:.2e} traces {got[2]:.2e} / {got[3]:.2e}")
        assert sa == sb and max(got) <= tol, (a, b, key, got)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("tree", bc.BATCH_TREES)
def test_batch_kernel_matches_oracle_from_crafted_starts(tree, dtype, monkeypatch):
    """k_cpb (double, and float under RAOCP_CPB_F32=1): B = 3 instances, each from its own crafted
    start and its own x0, each against its own oracle run. Both forms of the kernel by name: the
    golden problems' tables are staged in LDS (<true>), those of the 7-mode tree m7x32 exceed its
    budget and are read from HBM (<false>), in double and in float."""
    if dtype == "float32":
        monkeypatch.setenv("RAOCP_CPB_F32", "1")
    r, prob, op, alpha = bc.problem(tree)
    assert bc.rotations(tree) == 1
    f32 = dtype == "float32"
    nat = core.Cache(prob, dtype=dtype).native
    assert nat.kernel_info(13) == bc.BATCH_KERNEL[tree][f32]
    scales = (1.0, 0.5, 0.1)
    seeds = bc.BATCH_SEEDS[tree]
    X = np.stack([sc * np.asarray(r["x0"], dtype=float).reshape(-1) for sc in scales])
    Z0 = np.stack([bc.start(tree, 0, s, f32)[0] for s in seeds])
    E0 = np.stack([bc.start(tree, 0, s, f32)[1] for s in seeds])
    tol_z, tol_t = TOL[dtype]
    for K in bc.ITERS:
        status, errs, derrs = nat.cp_batch_run(X, K, 0.0, alpha, Z0, E0)
        for b, (sc, seed) in enumerate(zip(scales, seeds)):
            st_o, err_o, derr_o, z_o, e_o = bc.reference(tree, K, 0, seed, f32, sc)
            z, e = nat.cp_batch_get(b)
            assert int(status[b]) == st_o == 1 and errs[b].shape == err_o.shape == (K + 1, 3)
            got = (_seg_max(z, z_o, op, "primal"), _seg_max(e, e_o, op, "dual"), trace_rel_err(errs[b], err_o), trace_rel_err(derrs[b], derr_o))
            print(f"branches {nat.kernel_info(13)} {tree} instance {b} K {K}: primal {got[0]:.2e} dual {got[1]:.2e} "
                  f"traces {got[2]:.2e} / {got[3]:.2e}")
            assert np.isfinite(z).all() and np.isfinite(e).all()
            assert got[0] <= tol_z and got[1] <= tol_z, (tree, b, K, segment_rel_err(z, z_o, op, "primal"), segment_rel_err(e, e_o, op, "dual"))
            assert got[2] <= tol_t and got[3] <= tol_t, (tree, b, K, got)


@pytest.mark.parametrize("tree", bc.ENTRY_TREES)
def test_stand_alone_prox_and_projections_on_crafted_dual(tree):
    """proximal_of_g_conjugate and the two projections applied once to a crafted dual (every
    branch taken: test_branch_census.py), against the oracle's methods at 1e-12 per segment,
    the suite's bound for a single application."""
    r, prob, op, alpha = bc.problem(tree)
    cache = core.Cache(prob)
    for rot in range(bc.rotations(tree)):
        d0 = bc.start(tree, rot, bc.ENTRY_SEEDS[tree])[1]
        v = d0 / alpha
        cache.set_dual_flat(d0)
        cache.proximal_of_g_conjugate(alpha)
        got = {"prox_gconj": _seg_max(cache.get_dual_flat(), op.prox_gconj(d0, alpha), op, "dual")}
        cache.set_dual_flat(v)
        cache.project_on_constraints_nonleaf()
        got["project_nonleaf"] = _seg_max(cache.get_dual_flat(), op.project_on_constraints_nonleaf(v), op, "dual")
        cache.set_dual_flat(v)
        cache.project_on_constraints_leaf()
        got["project_leaf"] = _seg_max(cache.get_dual_flat(), op.project_on_constraints_leaf(v), op, "dual")
        print(f"branches entry points {tree} rot {rot}:", {k: f"{x:.2e}" for k, x in got.items()})
        assert max(got.values()) <= 1e-12, got


@pytest.mark.parametrize("tree", bc.TIE_TREES)
def test_projection_ties(tree):
    """The edges of the comparisons, through the stand-alone projections (one application, no
    rounding upstream): F = 0 with t > 0, = 0, < 0; nf == t and nf == -t exactly; box entries
    exactly at lo and at hi. Against the oracle at 1e-12 per segment; finite everywhere (v / nf is
    not evaluated where nf = 0); and since neither the identity nor the zero branch computes
    anything, those cones come back bit for bit: the input where nf <= t, zeros where nf <= -t."""
    r, prob, op, alpha = bc.problem(tree)
    cache = core.Cache(prob)
    v, child, ckeep, leaf, lkeep = bc.tie_dual(tree)
    cache.set_dual_flat(v)
    cache.project_on_constraints_nonleaf()
    got_nl = cache.get_dual_flat()
    cache.set_dual_flat(v)
    cache.project_on_constraints_leaf()
    got_l = cache.get_dual_flat()
    assert np.isfinite(got_nl).all() and np.isfinite(got_l).all()
    ref_nl, ref_l = op.project_on_constraints_nonleaf(v), op.project_on_constraints_leaf(v)
    assert _seg_max(got_nl, ref_nl, op, "dual") <= 1e-12, segment_rel_err(got_nl, ref_nl, op, "dual")
    assert _seg_max(got_l, ref_l, op, "dual") <= 1e-12, segment_rel_err(got_l, ref_l, op, "dual")
    for got, idx, keep in ((got_nl, child, ckeep), (got_l, leaf, lkeep)):
        assert np.array_equal(got[idx[keep]], v[idx[keep]])  # F = 0 with t >= 0, nf == t: the identity
        assert not got[idx[~keep]].any()                     # F = 0 with t < 0, nf == -t: zero
