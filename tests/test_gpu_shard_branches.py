"""GPU: the sharded path from crafted warm starts, on dense inputs, over the whole owned iterate.

tests/test_gpu_shard.py holds the sharded solve to the unsharded one on cold starts of the
recipe_config trees and compares the owned x alone. The code only a shard runs (k_cp3 as two
launches with the cut's parents reading their children's eta2 from X1; k_cp5's range lists and its
second family launch; the CP blocks, tier launches and per-stage sweeps over owned ranges; the X1 /
X2 pack and unpack) therefore never saw an identity or zero cone, a value outside its box or a
negative eta2 at a cut root, nor a dense weight table. Here every case of branch_cases.SHARDED runs
R shards on one device (group_cp_run with warm=True) for one and for three iterations from the
tree's crafted start, set whole on every shard (the entries a shard does not own are then stale by
design and are masked out: helpers.shard_masks; tests/test_dist_cpu.py proves the masks leave no
live entry out). tests/test_branch_census.py proves, with the oracle alone, that the start takes
every branch at the cut stage itself.

Each shard's kernel_info is asserted, so a fallback to another kernel fails. Bounds: TOL of
tests/test_gpu_branches.py against the oracle, per segment over the shard's mask; bit for bit
against the unsharded context on the same kernels from the same start (traces, masked primal and
dual), and between the shards' copies of the replicated top. The largest errors seen on an MI355X
are in profiles/r14_shard_branches/README.md.
"""
import numpy as np
import pytest

import raocp.core as core
from raocp.core._native import group_cp_run
import branch_cases as bc
from helpers import masked_segment_rel_err, shard_masks, shard_ranges, shard_top_masks, trace_rel_err
from test_gpu_branches import TOL, _env

pytestmark = pytest.mark.gpu

_PARAMS = [(c[0], R) for c in bc.SHARDED for R in c[6]]


def _assert_info(nat, info, who):
    for which, how, text in info:
        got = nat.kernel_info(which)
        ok = {"eq": got == text, "starts": got.startswith(text), "has": text in got}[how]
        assert ok, (who, which, how, text, got)


def _contexts(case, R):
    """The unsharded context and the R shards of a case, created under its environment (R = 1: one
    forced shard, which runs the exchange path alone), each shard's kernels and cut asserted."""
    _, tree, env, dtype, info, how, _ = bc.SHARDED_CASE[case]
    r, prob, op, alpha = bc.problem(tree)
    S = bc.shard_cut(tree, how, R)
    assert S is not None, (case, R, "the host rule says shard setup refuses this R")
    with _env(dict(env, RAOCP_SHARD_FORCE="1") if R == 1 else env):
        base = core.Cache(prob, dtype=dtype)
        shards = [core.Cache(prob, dtype=dtype) for _ in range(R)]
        for k, s in enumerate(shards):
            s.native.shard(k, R)
    want = shard_ranges(op, S, R)
    for k, s in enumerate(shards):
        _assert_info(s.native, info, (case, R, k))
        lo, hi = s.native.shard_owned()
        assert np.array_equal(lo, want[k][0]) and np.array_equal(hi, want[k][1]), (case, R, k, S, lo, hi, want[k])
    # the unsharded context runs the same CP kernel family (its fused forms in one launch)
    b10, s10 = base.native.kernel_info(10), shards[0].native.kernel_info(10)
    assert b10.split("<")[0] == s10.split("<")[0], (b10, s10)
    return base, shards, S


def _start(cache, p0, d0):
    cache.set_primal_flat(p0)
    cache.set_dual_flat(d0)


@pytest.mark.parametrize("case,R", _PARAMS, ids=[f"{c}-R{R}" for c, R in _PARAMS])
def test_shards_match_oracle_and_unsharded_from_crafted_start(case, R):
    _, tree, env, dtype, info, how, _ = bc.SHARDED_CASE[case]
    r, prob, op, alpha = bc.problem(tree)
    f32 = dtype == "float32"
    tol_z, tol_t = TOL[dtype]
    seed = bc.shard_seed_of(tree)
    base, shards, S = _contexts(case, R)
    own = [s.native.shard_owned() for s in shards]
    masks = [shard_masks(op, lo, hi, S) for lo, hi in own]
    top_p, top_d = shard_top_masks(op, S)
    assert top_p.any() and top_d.any() and all((pm & top_p).sum() == top_p.sum() and (dm & top_d).sum() == top_d.sum()
                                               for pm, dm in masks)
    worst = np.zeros(4)
    for rot in range(bc.rotations(tree)):
        p0, d0, _, _ = bc.start(tree, rot, seed, f32)
        for K in bc.ITERS:
            st_o, err_o, derr_o, z_o, e_o = bc.reference(tree, K, rot, seed, f32)
            _start(base, p0, d0)
            st_b, err_b, derr_b = base.native.cp_run(r["x0"], K, 0.0, alpha, warm=True)
            z_b, e_b = base.get_primal_flat(), base.get_dual_flat()
            for s in shards:
                _start(s, p0, d0)
            st, err, derr = group_cp_run([s.native for s in shards], r["x0"], K, 0.0, alpha, warm=True)
            assert st == st_b == st_o == 1 and err.shape == err_o.shape == (K + 1, 3) and derr.shape == derr_o.shape
            got = [0.0, 0.0, trace_rel_err(err, err_o), trace_rel_err(derr, derr_o)]
            zs, es = [s.get_primal_flat() for s in shards], [s.get_dual_flat() for s in shards]
            for k, (pm, dm) in enumerate(masks):
                assert np.isfinite(zs[k][pm]).all() and np.isfinite(es[k][dm]).all(), (case, R, k, rot, K)
                seg_p = masked_segment_rel_err(zs[k], z_o, op, "primal", pm)
                seg_d = masked_segment_rel_err(es[k], e_o, op, "dual", dm)
                got[0], got[1] = max(got[0], *seg_p.values()), max(got[1], *seg_d.values())
                assert max(seg_p.values()) <= tol_z and max(seg_d.values()) <= tol_z, (case, R, k, rot, K, seg_p, seg_d)
            print(f"shard-branches {case} R {R} rot {rot} K {K}: primal {got[0]:.2e} dual {got[1]:.2e} "
                  f"traces {got[2]:.2e} / {got[3]:.2e}")
            worst = np.fmax(worst, got)
            assert got[2] <= tol_t and got[3] <= tol_t, (case, R, rot, K, got)
            # the unsharded context on the same kernels, from the same start: bit for bit
            assert np.array_equal(err, err_b) and np.array_equal(derr, derr_b), (case, R, rot, K, err, err_b, derr, derr_b)
            for k, (pm, dm) in enumerate(masks):
                bad_p, bad_d = np.flatnonzero(pm & (zs[k] != z_b)), np.flatnonzero(dm & (es[k] != e_b))
                assert bad_p.size == 0 and bad_d.size == 0, (case, R, k, rot, K, bad_p[:8], bad_d[:8])
            # the shards' copies of the replicated top: bit for bit
            for k in range(1, R):
                assert np.array_equal(zs[k][top_p], zs[0][top_p]) and np.array_equal(es[k][top_d], es[0][top_d]), (case, R, k)
    print(f"shard-branches-max {case} R {R}: primal {worst[0]:.2e} dual {worst[1]:.2e} traces {worst[2]:.2e} / {worst[3]:.2e}")


def test_cold_group_run_after_a_warm_one_is_the_cold_run():
    """The warm flag leaves no state behind: group_cp_run(..., warm=False) after a warm run from the
    crafted start reproduces, bit for bit, the cold run of the same shards before it (traces and
    every shard's masked primal and dual)."""
    case, R, K = "sh-cp3-bin8-dense", 3, 3
    _, tree, env, dtype, info, how, _ = bc.SHARDED_CASE[case]
    r, prob, op, alpha = bc.problem(tree)
    base, shards, S = _contexts(case, R)
    masks = [shard_masks(op, *s.native.shard_owned(), S) for s in shards]
    nats = [s.native for s in shards]

    def cold():
        st, err, derr = group_cp_run(nats, r["x0"], K, 0.0, alpha)
        return st, err, derr, [s.get_primal_flat() for s in shards], [s.get_dual_flat() for s in shards]

    st0, err0, derr0, z0, e0 = cold()
    p0, d0, _, _ = bc.start(tree, 0, bc.shard_seed_of(tree))
    for s in shards:
        _start(s, p0, d0)
    _, err_w, _ = group_cp_run(nats, r["x0"], K, 0.0, alpha, warm=True)
    assert not np.array_equal(err_w, err0)  # the warm run did start elsewhere
    st1, err1, derr1, z1, e1 = cold()
    assert st1 == st0 and np.array_equal(err1, err0) and np.array_equal(derr1, derr0)
    for k, (pm, dm) in enumerate(masks):
        assert np.array_equal(z1[k][pm], z0[k][pm]) and np.array_equal(e1[k][dm], e0[k][dm]), k
