"""CPU: the crafted warm starts of tests/branch_cases.py take every branch of the dual step in
their first CP iteration, by the oracle's own census (OracleProblem.branch_census), and the
per-segment comparison notices a wrong branch.

These are conditions on the test inputs, not measurements: tests/test_gpu_branches.py pins the
cone and box branches of every CP kernel only if its starts reach them, clear of the comparisons'
edges (a margin of 0.1 cannot flip under fp32 rounding of the norm, 1e-6).
"""
import numpy as np
import pytest

import branch_cases as bc
from helpers import segment_rel_err


def _forced_classes_taken(c, ccls, lcls):
    """A cone built for the identity or the zero class takes it (one left at its random value is
    usually scaling, not always: the shares below count what the oracle took, not what was meant)."""
    for got, want in ((c["child_class"], ccls), (c["leaf_class"], lcls)):
        assert np.array_equal(got[want != 2], want[want != 2])


@pytest.mark.parametrize("tree,seed", bc.CENSUS_CASES, ids=[f"{t}-{s}" for t, s in bc.CENSUS_CASES])
def test_crafted_start_takes_every_branch(tree, seed):
    """Iteration 1 of chock from the crafted start(s) of a tree: each SOC class on >= 30 % of the
    child cones and of the leaf cones, every margin >= 0.1, every (child slot, class) pair, each
    box branch on >= 5 % of the boxed entries, each sign on >= 10 % of the clamped eta1 / eta2
    entries (branch_cases.census_violations)."""
    r, prob, op, alpha = bc.problem(tree)
    rots = range(bc.rotations(tree))
    cens = [bc.census(tree, rot, seed) for rot in rots]
    for rot, c in zip(rots, cens):
        _forced_classes_taken(c, *bc.start(tree, rot, seed)[2:])
        print(tree, seed, rot, "child", np.bincount(c["child_class"], minlength=3).tolist(), f"{c['child_margin'].min():.3f}",
              "leaf", np.bincount(c["leaf_class"], minlength=3).tolist(), f"{c['leaf_margin'].min():.3f}",
              "box_nl", c["box_nl"].tolist(), "box_l", c["box_l"].tolist(),
              "eta1", c["eta1_sign"].tolist(), "eta2", c["eta2_sign"].tolist())
    assert bc.census_violations(op, cens, bc.box_exempt(tree)) == []
    # an exempted kind of box is a real exception, not a convenience: no entry leaves it
    for key in bc.box_exempt(tree):
        assert all(c[key][:2].sum() == 0 and c[key][2] > 0 for c in cens)


def test_box_exemption_is_main_leaf_box_only():
    """The one exception to the per-kind box condition: golden main's leaf box (+-7 on a state of
    order 1, out of reach of a standard normal start). The leaf-box code of the kernels main runs
    is reached, under the full condition, on bin7 (scalar) and on bin6 and c1n5 (batch)."""
    assert bc.BOX_EXEMPT == {"main": ("box_l",)}
    assert bc.FAMILY["scalar-bin7"][2] == bc.FAMILY["scalar-main"][2]
    assert {"bin6", "c1n5"} <= set(bc.BATCH_TREES) and not bc.box_exempt("bin6") and not bc.box_exempt("c1n5")
    for tree in ("bin7", "bin6", "c1n5"):
        assert bc.problem(tree)[2].l_active.all()


@pytest.mark.parametrize("tree", ["bin7", "main", "chain12", "m7x32"])
def test_census_dual_is_the_one_chock_projects(tree):
    """chock_modified_duals restates chock's loop to expose v; this ties the two together: the
    Moreau step alpha (v - Pi(v)) of the last v it returns is chock's returned dual, bit for
    bit, after one iteration and after three."""
    r, prob, op, alpha = bc.problem(tree)
    p0, d0, _, _ = bc.start(tree, 0, bc.seed_of(tree))
    for K in bc.ITERS:
        vs = op.chock_modified_duals(r["x0"], K, alpha, p0=p0, d0=d0)
        assert len(vs) == K + 1
        v = vs[-1]
        proj = op.project_on_constraints_leaf(op.project_on_constraints_nonleaf(v))
        assert np.array_equal(alpha * (v - proj), bc.reference(tree, K, 0, bc.seed_of(tree))[4])
    # and a cold start
    v = op.chock_modified_duals(r["x0"], 0, alpha)[0]
    e = op.chock(r["x0"], 0, 0.0, alpha=alpha)[4]
    assert np.array_equal(alpha * (v - op.project_on_constraints_leaf(op.project_on_constraints_nonleaf(v))), e)


@pytest.mark.parametrize("tree", bc.ENTRY_TREES)
def test_entry_point_inputs_take_every_branch(tree):
    """The stand-alone entry points project the crafted dual itself: prox g* sees
    modify_dual_add_halves(d0, alpha), the two projections d0 / alpha. The same conditions hold
    for both (the eta1 / eta2 signs and the boxes per kind included, but for main's leaf box:
    branch_cases.BOX_EXEMPT)."""
    r, prob, op, alpha = bc.problem(tree)
    seed = bc.ENTRY_SEEDS[tree]
    rots = range(bc.rotations(tree))
    for v_of in (lambda d0: op.modify_dual_add_halves(d0, alpha), lambda d0: d0 / alpha):
        cens = [op.branch_census(v_of(bc.start(tree, rot, seed)[1])) for rot in rots]
        for rot, c in zip(rots, cens):
            _forced_classes_taken(c, *bc.start(tree, rot, seed)[2:])
        assert bc.census_violations(op, cens, bc.box_exempt(tree)) == []


def test_the_conditions_reject_a_cold_start():
    """What the crafted start is for: iteration 1 of a cold start (and a random warm start
    without the cone offsets) misses the class shares on the same tree."""
    r, prob, op, alpha = bc.problem("bin7")
    cold = op.branch_census(op.chock_modified_duals(r["x0"], 0, alpha)[0])
    assert any("cone classes" in b for b in bc.census_violations(op, [cold]))
    rng = np.random.default_rng(0)
    v = op.chock_modified_duals(r["x0"], 0, alpha, p0=rng.standard_normal(op.P), d0=alpha * rng.standard_normal(op.D))[0]
    assert any("cone classes" in b for b in bc.census_violations(op, [op.branch_census(v)]))


def test_census_is_the_branch_soc_takes():
    """branch_census classifies by _soc's own comparisons: on random rows and on the ties
    (nf == t, nf == -t, nf == 0) the class decides what _soc returns."""
    from oracle.raocp_oracle import OracleProblem
    rng = np.random.default_rng(3)
    F = rng.standard_normal((64, 5))
    t = rng.standard_normal(64) * 3
    F[:6] = 0.0
    F[6:12] = [3.0, 4.0, 0.0, 0.0, 0.0]
    t[:12] = [1.0, 0.0, -1.0, 0.0, 2.0, -2.0, 5.0, -5.0, 5.0, -5.0, 4.0, -4.0]
    cls, margin = OracleProblem._soc_class(F, t)
    oF, ot = OracleProblem._soc(F, t)
    assert np.isfinite(oF).all() and np.isfinite(ot).all() and np.isfinite(margin).all()
    assert set(cls.tolist()) == {0, 1, 2}
    assert np.array_equal(oF[cls == 0], F[cls == 0]) and np.array_equal(ot[cls == 0], t[cls == 0])
    assert not oF[cls == 1].any() and not ot[cls == 1].any()
    nf = np.linalg.norm(F, axis=1)
    assert np.allclose(ot[cls == 2], (nf[cls == 2] + t[cls == 2]) / 2, rtol=0, atol=1e-15)
    # F = 0: t >= 0 identity, t < 0 zero; nf == t identity, nf == -t zero
    assert cls[:12].tolist() == [0, 0, 1, 0, 0, 1, 0, 1, 0, 1, 2, 2]
    assert margin[6] == margin[7] == 0.0


@pytest.mark.parametrize("tree", bc.TIE_TREES)
def test_tie_dual_sits_on_the_edges(tree):
    """The oracle's reading of the ties the GPU test holds the kernels to (cones.py:113-132:
    nf <= t first, then nf <= -t): the cones meant to pass come back bit for bit, the others are
    zeroed, every margin is exactly 0 or the cone has F = 0, and nothing is NaN."""
    r, prob, op, alpha = bc.problem(tree)
    v, child, ckeep, leaf, lkeep = bc.tie_dual(tree)
    c = op.branch_census(v)
    assert np.array_equal(c["child_class"] == 0, ckeep) and np.array_equal(c["child_class"] == 1, ~ckeep)
    assert np.array_equal(c["leaf_class"] == 0, lkeep) and np.array_equal(c["leaf_class"] == 1, ~lkeep)
    for idx, margin in ((child, c["child_margin"]), (leaf, c["leaf_margin"])):
        nf = np.linalg.norm(v[idx[:, :-1]], axis=1)
        assert np.all((margin == 0.0) | (nf == 0.0)) and set(nf.tolist()) <= {0.0, 5.0}
    for ref, idx, keep in ((op.project_on_constraints_nonleaf(v), child, ckeep), (op.project_on_constraints_leaf(v), leaf, lkeep)):
        assert np.isfinite(ref).all()
        assert np.array_equal(ref[idx[keep]], v[idx[keep]]) and not ref[idx[~keep]].any()
    if c["box_nl"].sum():
        assert c["box_nl"][:2].min() >= c["box_nl"].sum() // 3 - op.m


def test_live_masks_are_what_the_loop_writes():
    """The live slots are exactly those L (dual) and L^T (primal) write over a template, on
    trees with every box pattern; a crafted start is zero on the others and a CP iteration
    keeps them zero."""
    for tree in ("bin7", "bin7-leafbox", "bin7-nobox", "main", "chain12"):
        r, prob, op, alpha = bc.problem(tree)
        pm, dm = op.live_masks()
        rng = np.random.default_rng(1)
        assert np.array_equal(np.isfinite(op.ell(rng.standard_normal(op.P), template=np.full(op.D, np.nan))), dm)
        assert np.array_equal(np.isfinite(op.ell_t(rng.standard_normal(op.D), template=np.full(op.P, np.nan))), pm)
        p0, d0, _, _ = bc.start(tree, 0, bc.seed_of(tree))
        assert not p0[~pm].any() and not d0[~dm].any() and p0[pm].all() and d0[dm].all()
        zp, ep, _, _ = op.cp_iteration(p0, d0, alpha, r["x0"])
        assert not zp[~pm].any() and not ep[~dm].any()


@pytest.mark.parametrize("tree", ["bin7", "main"])
def test_segment_rel_err_sees_a_swapped_branch(tree, monkeypatch):
    """The harness notices a wrong branch: an oracle whose _soc returns zero where it should
    return the input and the input where it should return zero differs from the true one by
    more than 1e-2 in every cone segment (eta3..eta6, eta11..eta13), per segment."""
    from oracle.raocp_oracle import OracleProblem
    r, prob, op, alpha = bc.problem(tree)
    p0, d0, _, _ = bc.start(tree, 0, bc.seed_of(tree))
    st, err, derr, z, e = bc.reference(tree, 0, 0, bc.seed_of(tree))
    true_soc = OracleProblem._soc

    def swapped(F, t):
        nf = np.linalg.norm(F, axis=1)
        oF, ot = true_soc(F, t)
        ident = nf <= t
        zero = (nf > t) & (nf <= -t)
        oF[ident], ot[ident] = 0.0, 0.0
        oF[zero], ot[zero] = F[zero], t[zero]
        return oF, ot

    monkeypatch.setattr(OracleProblem, "_soc", staticmethod(swapped))
    _, _, _, z_m, e_m, _ = op.chock(r["x0"], 0, 0.0, alpha=alpha, p0=p0, d0=d0)
    monkeypatch.undo()
    seg = segment_rel_err(e_m, e, op, "dual")
    print(tree, {k: f"{v:.2e}" for k, v in seg.items()})
    for name in ("eta3", "eta4", "eta5", "eta6", "eta11", "eta12", "eta13"):
        assert seg[name] > 1e-2, (name, seg[name])
    # and an unmutated rerun is exactly the reference
    _, _, _, z2, e2, _ = op.chock(r["x0"], 0, 0.0, alpha=alpha, p0=p0, d0=d0)
    assert max(segment_rel_err(e2, e, op, "dual").values()) == 0.0 and max(segment_rel_err(z2, z, op, "primal").values()) == 0.0


def test_segment_rel_err_takes_the_kind_it_is_told():
    """Told apart by length only where the lengths differ; a kind that does not fit the vector is
    refused, and where primal and dual have one length the kind must be given."""
    import types
    r, prob, op, alpha = bc.problem("bin3")
    z, e = np.ones(op.P), np.ones(op.D)
    assert list(segment_rel_err(z, z, op)) == list(segment_rel_err(z, z, op, "primal")) == ["x", "u", "y", "tau", "s"]
    assert list(segment_rel_err(e, e, op))[0] == "eta1"
    with pytest.raises(AssertionError):
        segment_rel_err(z, z, op, "dual")
    same = types.SimpleNamespace(P=op.D, D=op.D, d_off=op.d_off, X0=0, U0=1, Y0=2, T0=3, S0=4)
    with pytest.raises(AssertionError):
        segment_rel_err(e, e, same)
    assert list(segment_rel_err(e, e, same, "primal")) == ["x", "u", "y", "tau", "s"]


@pytest.mark.parametrize("tree", bc.SHARD_TREES)
def test_crafted_start_takes_every_branch_at_the_cut(tree):
    """The code only a shard runs sits at the cut stage S and at its parents; the tree-wide census
    does not say where its classes fall. At every cut the sharded cases of the tree use (the tier
    planner's cut on the host, or the first stage with 8 R nodes: branch_cases.shard_cut, which the
    GPU test holds against raocp_shard_owned), iteration 1 from the sharded cases' start takes every
    cone class among the child cones of the stage-S nodes and among those of their children, both
    signs under the clamp of the roots' eta2 (the entries X1 carries) over the stage and within
    every shard's slice of >= 4 roots, and a lo and a hi branch in the cut's parents' boxes
    (branch_cases.cut_census_violations); the tree-wide conditions, margins included, hold for the
    same seed (CENSUS_CASES)."""
    r, prob, op, alpha = bc.problem(tree)
    seed = bc.shard_seed_of(tree)
    assert (tree, seed) in bc.CENSUS_CASES
    cuts = bc.shard_cuts(tree)
    assert cuts and None not in cuts, cuts
    vs = [bc.modified_dual(tree, rot, seed) for rot in range(bc.rotations(tree))]
    for S, Rs in sorted(cuts.items()):
        print(tree, "seed", seed, "cut", S, "R", sorted(Rs))
        assert bc.cut_census_violations(op, vs, S, sorted(Rs)) == []


def test_sharded_table_meets_the_required_shard_counts():
    """Every sharded case runs at least R = 2; the two-tier binary tree's rows include R = 3 (16
    roots at the cut: 5 / 5 / 6); a ternary case includes R = 2; the R values listed are exactly
    those of 1, 2, 3, 4, 8 the host rule of shard setup accepts."""
    for cid, tree, env, dtype, info, how, Rs in bc.SHARDED:
        assert 2 in Rs, cid
        assert tuple(R for R in (1, 2, 3, 4, 8) if bc.shard_cut(tree, how, R) is not None) == Rs, cid
        if tree.startswith("bin8"):
            assert 3 in Rs and bc.shard_cut(tree, how, 3) == 4
    assert any(c[1].startswith("tern") and 2 in c[6] for c in bc.SHARDED)


def test_the_cut_conditions_reject_the_seed_they_replaced():
    """What the sharded cases' own seeds are for: on bin8 the tree's seed leaves a shard's slice of
    the roots with one sign of eta2, and a cold start misses the cone classes at the cut."""
    r, prob, op, alpha = bc.problem("bin8")
    v = bc.modified_dual("bin8", 0, bc.seed_of("bin8"))
    assert any("one sign" in b for b in bc.cut_census_violations(op, [v], 4, [3, 4]))
    cold = op.chock_modified_duals(r["x0"], 0, alpha)[0]
    assert any("cone classes" in b for b in bc.cut_census_violations(op, [cold], 4, [2]))
