"""GPU: the runtime-size kernels <0, 0> and every MFMA tile instantiation <rx, ru> on general
problems (raocp.problems.recipe_general: dense weight tables, a bound of its own per box entry with
one-sided entries, risk levels 0.1 / 0.7 / 0.99), at the shapes where a tile kernel can go wrong,
against the oracle, in fp64 and fp32.

Shapes (branch_cases.SHAPES; trees of 31, 40 or 121 nodes) and the cell (rx, ru) =
(ceil(nx / 16), ceil(nu / 16)) of dispatch_rt (raocp_capi.hip) each one reaches:

    (1, 1)    <1, 1>  the minimum, odd        (24, 17)  <2, 2>  ru = 2 with a one-row tail
    (5, 3)    <1, 1>  odd / odd               (33, 7)   <3, 1>  rx = 3, tail 1
    (6, 18)   <1, 2>  ru = 2 at rx = 1        (48, 32)  <3, 2>  full tiles
    (16, 16)  <1, 1>  exactly one full tile   (49, 9)   <4, 1>  rx = 4, tail 1
    (17, 5)   <2, 1>  rx = 2, tail 1          (64, 32)  <4, 2>  the admitted maximum

Which case names which kernel (every string is asserted through kernel_info):
  - k_cpd2 / k_cpp2<double, rx, ru> and <float, rx, ru>: test_cp_kernels[mfma] on the shape's tree
    with one weight table ("s<nx>x<nu>u"): all eight cells, both types; k_ell2 / k_ellt2<float, rx, ru>:
    every fp32 case on a one-table tree (with a table per mode an fp32 context refuses L and L^T,
    asserted); the k_d2_* tiles <float>: every fp32 case;
  - k_cpd / k_cpp<double, 0, 0> and <float, 0, 0>: test_cp_kernels[auto] on the tree with a table per
    mode (the node blocks mix tables, so fp32 leaves the MFMA kernels too) and [scalar] on the
    one-table tree; k_ell / k_ell_t<0, 0>: every fp64 case;
  - a table per mode under RAOCP_CP_V1=0 RAOCP_CP3=0: the MFMA kernels take one table per
    block, so the library runs the scalar ones; test_mfma_setting_falls_back_with_a_table_per_mode
    asserts that fallback;
  - the dynamics: k_dyn_top<0, 0, .., ..> alone (nx <= 24), k_dyn_up / k_dyn_down<0, 0> (33, 7),
    k_dyn_bottom_back / _fwd<0, 0, ..> with one tier (48, 32), (49, 9) and two (64, 32) by
    default; test_dynamics_engines adds the per-stage fallback, the split sweep's selection
    (RAOCP_DR=0; it runs at (33, 7) and reports the tier launches elsewhere), the tier launches
    (RAOCP_DYN_SPLIT=0) and k_d2_*<double> (RAOCP_DYN2=1) on odd and even shapes;
  - k_cpb<true>, k_cpb<float, true>, k_mpc_step and k_mpc_step<float>: test_batch_and_mpc.

Bounds are the suite's own. fp64: 1e-12 operators and projections, 1e-11 dynamics and prox f, 1e-8
per trace entry, 1e-10 on the iterate (test_gpu_parity.py). fp32: 2e-6 one operator application
(test_gpu_fp32.TOL32), 2e-5 the dynamics projection and prox f (its bound at config 5), 1e-4 / 1e-5
traces / iterate of a cold run (its bounds for 30 iterations, used here for 10), and from a crafted
start 2e-4 per segment and 2e-3 per trace entry (test_gpu_branches.TOL).
"""
import contextlib
import os

import numpy as np
import pytest

import raocp.core as core
from raocp.core._native import RaocpError
from raocp.problems import build_problem, recipe_general
import branch_cases as bc
from helpers import rel_err, segment_rel_err, trace_rel_err

pytestmark = pytest.mark.gpu

SHAPES = list(bc.SHAPES)
DTYPES = ["float64", "float32"]
CP_ENV = {"auto": {}, "scalar": {"RAOCP_CP_V1": "1"}, "mfma": {"RAOCP_CP_V1": "0", "RAOCP_CP3": "0"}}
DYN_ENV = {"default": {}, "per_stage": {"RAOCP_DYN_PER_STAGE": "1"}, "split": {"RAOCP_DR": "0"},
           "tiers": {"RAOCP_DYN_SPLIT": "0", "RAOCP_DR": "0"}, "dyn2": {"RAOCP_DYN2": "1"}}
_TOP, _TOPNF = "k_dyn_top<0, 0, true, true> x1", "k_dyn_top<0, 0, true, false> x1"
_T1 = "k_dyn_bottom_back<0, 0, false> x1 + k_dyn_top<0, 0, false, false> x1 + k_dyn_bottom_fwd<0, 0, {}> x1"
# the launches of the tier plan of each shape's tree (fp64), and where the split sweep takes them over
TIERS = {(1, 1): _TOP, (5, 3): _TOP, (6, 18): _TOP, (16, 16): _TOP, (17, 5): _TOP, (24, 17): _TOPNF,
         (33, 7): "k_dyn_bottom_back<0, 0, true> x1 + k_dyn_top<0, 0, true, true> x1 + k_dyn_bottom_fwd<0, 0, 1> x1",
         (48, 32): _T1.format(1), (49, 9): _T1.format(2),
         (64, 32): "k_dyn_bottom_back<0, 0, false> x1 + k_dyn_bottom_back<0, 0, true> x1 + k_dyn_top<0, 0, false, true> x1 + "
                   "k_dyn_bottom_fwd<0, 0, 1> x1 + k_dyn_bottom_fwd<0, 0, 2> x1"}
SPLIT = {(33, 7): "k_dyn_up<0, 0> x1 + k_dyn_down<0, 0, true> x1"}
PER_STAGE = "k_dyn_gather + k_dyn_stage_a / _b / _f (per stage)"
DYN2 = "k_d2_prod + k_d2_node + k_d2_x0 + k_d2_fwd (per stage, {})"
# fp64 / fp32: one application of an operator or projection; the dynamics projection and prox f; traces and iterate
# of a cold run; segments and traces from a crafted start
TOL = {"float64": dict(op=1e-12, dyn=1e-11, feas=1e-10, adj=1e-10, trace=1e-8, z=1e-10, seg=1e-10, ctrace=1e-8),
       "float32": dict(op=2e-6, dyn=2e-5, feas=1e-5, adj=1e-5, trace=1e-4, z=1e-5, seg=2e-4, ctrace=2e-3)}
K_COLD, K_CRAFTED = 9, 2  # max_iters: 10 iterations from x0, 3 from the crafted start


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


def _cell(nx, nu):
    return f"{min(4, (nx + 15) // 16)}, {1 if nu <= 16 else 2}"


def _t(dtype):
    return "double" if dtype == "float64" else "float"


def _scalar(dtype):
    return f"k_cpd<{_t(dtype)}, 0, 0> + k_cpp<{_t(dtype)}, 0, 0>"


def _mfma(nx, nu, dtype):
    return f"k_cpd2<{_t(dtype)}, {_cell(nx, nu)}> + k_cpp2<{_t(dtype)}, {_cell(nx, nu)}>"


def _dyn_info(nx, nu, dtype, engine):
    if dtype == "float32" or engine == "dyn2":
        return DYN2.format(_t(dtype))
    if engine == "per_stage":
        return PER_STAGE
    if engine == "tiers":
        return TIERS[(nx, nu)]
    return SPLIT.get((nx, nu), TIERS[(nx, nu)])


_REF = {}


def _cold_reference(tree):
    """OracleProblem.chock from x0 for K_COLD iterations at the oracle's step size (once per tree)."""
    if tree not in _REF:
        r, prob, op, alpha = bc.problem(tree)
        _REF[tree] = op.chock(r["x0"], K_COLD, 0.0, alpha=alpha)[:5]
    return _REF[tree]


def _check_case(tree, nx, nu, dtype, env, cp_info, dyn_info):
    """Every check of a case on one context: the kernels by name, L / L^T and their adjoint
    identity, the two projections (with feasibility of the dynamics), prox f, prox g* (fp64; an
    fp32 context refuses the last three by contract, which is asserted), 10 CP iterations from
    x0 and 3 from the crafted start."""
    r, prob, op, alpha = bc.problem(tree)
    tol, f32 = TOL[dtype], dtype == "float32"
    with _env(env):
        cache = core.Cache(prob, dtype=dtype)
    nat = cache.native
    ell = (f"k_ell2<float, {_cell(nx, nu)}>", f"k_ellt2<float, {_cell(nx, nu)}>") if f32 else ("k_ell<0, 0>", "k_ell_t<0, 0>")
    got = tuple(nat.kernel_info(k) for k in (0, 1, 10, 9, 11))
    assert got == ell + (cp_info, dyn_info, ""), (tree, dtype, env, got)
    rng = np.random.default_rng(100 * nx + nu)
    zz, ee = rng.standard_normal(op.P), rng.standard_normal(op.D)
    x0 = np.asarray(r["x0"], dtype=float).reshape(-1)
    fig = {}
    # (by the packed tables: equal weights of several modes are one table to the library)
    if f32 and max(cache.packed.sqrt_q.shape[0], cache.packed.sqrt_r.shape[0]) > 1:
        # k_ell2 / k_ellt2<float> hold one weight fragment per node block: with a table per mode
        # an fp32 context refuses L, L^T and the step size built on them (it read the table at
        # index -1 and returned garbage before this module found it); its CP loop runs below
        for call in (lambda: nat.ell(zz), lambda: nat.ell_t(ee), nat.step_size):
            with pytest.raises(RaocpError, match="fp32 L / L\\^T need one weight table per node block"):
                call()
        fig["adjoint"] = 0.0
    else:
        lz, lte = nat.ell(zz), nat.ell_t(ee)
        fig["ell"], fig["ell_t"] = rel_err(lz, op.ell(zz)), rel_err(lte, op.ell_t(ee))
        a, b = float(zz @ lte), float(lz @ ee)
        fig["adjoint"] = abs(a - b) / max(1.0, abs(a))
    cache.cache_initial_state(x0)
    nat.set_primal(zz)
    nat.project_on_dynamics()
    z1 = nat.get_primal()
    fig["dynamics"] = rel_err(z1, op.project_on_dynamics(zz, x0))
    X, U = z1[op.X0:op.U0].reshape(op.n, nx), z1[op.U0:op.Y0].reshape(op.m, nu)
    j = np.arange(1, op.n)
    pred = np.stack([op.A[op.iA[k]] @ X[op.anc[k]] + op.B[op.iB[k]] @ U[op.anc[k]] for k in j])
    fig["feasible"] = float(np.max(np.abs(X[j] - pred))) / max(1.0, float(np.max(np.abs(X))))
    assert np.array_equal(X[0], x0.astype(np.float32).astype(float) if f32 else x0)
    if f32:  # an fp32 context offers the CP loop, L / L^T and the dynamics projection; the rest it refuses
        for call in (nat.project_on_kernel, lambda: nat.prox_f(0.3), lambda: nat.prox_gconj(0.3)):
            with pytest.raises(RaocpError, match="not available on an fp32 context"):
                call()
    else:
        nat.set_primal(zz)
        nat.project_on_kernel()
        fig["kernel"] = rel_err(nat.get_primal(), op.project_on_kernel(zz))
        cache.set_primal_flat(zz)
        cache.proximal_of_f(0.3)
        fig["prox_f"] = rel_err(cache.get_primal_flat(), op.prox_f(zz, 0.3, x0))
        cache.set_dual_flat(ee)
        cache.proximal_of_g_conjugate(0.3)
        e1 = cache.get_dual_flat()
        fig["prox_gconj"] = rel_err(e1, op.prox_gconj(ee, 0.3))
        assert np.isfinite(e1).all()
    print(f"shapes {tree} {dtype} {env}:", {k: f"{v:.2e}" for k, v in fig.items()})
    for k in ("ell", "ell_t", "kernel", "prox_gconj"):
        assert fig.get(k, 0.0) <= tol["op"], (k, fig)
    assert fig["dynamics"] <= tol["dyn"] and fig.get("prox_f", 0.0) <= tol["dyn"] and fig["feasible"] <= tol["feas"], fig
    assert fig["adjoint"] <= tol["adj"], fig
    # 10 iterations from x0
    st, err, derr = nat.cp_run(x0, K_COLD, 0.0, alpha)
    st_o, err_o, derr_o, z_o, e_o = _cold_reference(tree)
    z, e = cache.get_primal_flat(), cache.get_dual_flat()
    cold = (trace_rel_err(err, err_o), trace_rel_err(derr, derr_o), rel_err(z, z_o), rel_err(e, e_o))
    print(f"shapes {tree} {dtype} {env} cold: traces {cold[0]:.2e} / {cold[1]:.2e} iterate {cold[2]:.2e} / {cold[3]:.2e}")
    assert st == st_o == 1 and err.shape == (K_COLD + 1, 3)
    assert cold[0] <= tol["trace"] and cold[1] <= tol["trace"] and cold[2] <= tol["z"] and cold[3] <= tol["z"], cold
    # 3 iterations from the crafted start: every cone and box branch (tests/test_branch_census.py)
    assert bc.rotations(tree) == 1
    seed = bc.seed_of(tree)
    p0, d0, _, _ = bc.start(tree, 0, seed, f32)
    cache.set_primal_flat(p0)
    cache.set_dual_flat(d0)
    st, err, derr = nat.cp_run(x0, K_CRAFTED, 0.0, alpha, warm=True)
    st_o, err_o, derr_o, z_o, e_o = bc.reference(tree, K_CRAFTED, 0, seed, f32)
    z, e = cache.get_primal_flat(), cache.get_dual_flat()
    sp, sd = segment_rel_err(z, z_o, op, "primal"), segment_rel_err(e, e_o, op, "dual")
    crafted = (max(sp.values()), max(sd.values()), trace_rel_err(err, err_o), trace_rel_err(derr, derr_o))
    print(f"shapes {tree} {dtype} {env} crafted: primal {crafted[0]:.2e} dual {crafted[1]:.2e} traces {crafted[2]:.2e} / {crafted[3]:.2e}")
    assert st == st_o == 1 and np.isfinite(z).all() and np.isfinite(e).all()
    assert crafted[0] <= tol["seg"] and crafted[1] <= tol["seg"], (sp, sd)
    assert crafted[2] <= tol["ctrace"] and crafted[3] <= tol["ctrace"], crafted


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("setting", list(CP_ENV))
@pytest.mark.parametrize("nx,nu", SHAPES, ids=[f"{a}x{b}" for a, b in SHAPES])
def test_cp_kernels(nx, nu, setting, dtype):
    """auto: what the library picks on the tree with a weight table per mode (the scalar
    kernels in either type: the trees are small and their node blocks mix tables). scalar and
    mfma: RAOCP_CP_V1=1 and RAOCP_CP_V1=0 RAOCP_CP3=0 on the tree with one dense table."""
    tree = bc.shape_tree(nx, nu, shared=setting != "auto")
    cp = _mfma(nx, nu, dtype) if setting == "mfma" else _scalar(dtype)
    _check_case(tree, nx, nu, dtype, CP_ENV[setting], cp, _dyn_info(nx, nu, dtype, "default"))


@pytest.mark.parametrize("dtype", DTYPES)
def test_auto_picks_mfma_in_fp32_on_one_table(dtype):
    """The library's own choice on a one-table tree: fp32 takes the MFMA kernels, fp64 the
    scalar ones (few tiles)."""
    nx, nu = 17, 5
    cp = _mfma(nx, nu, dtype) if dtype == "float32" else _scalar(dtype)
    _check_case(bc.shape_tree(nx, nu, True), nx, nu, dtype, {}, cp, _dyn_info(nx, nu, dtype, "default"))


@pytest.mark.parametrize("dtype", DTYPES)
def test_mfma_setting_falls_back_with_a_table_per_mode(dtype):
    """RAOCP_CP_V1=0 RAOCP_CP3=0 on a tree whose blocks mix weight tables: k_cpd2 / k_cpp2 take one
    table per block, so the scalar kernels run and kernel_info says so."""
    nx, nu = 24, 17
    _check_case(bc.shape_tree(nx, nu), nx, nu, dtype, CP_ENV["mfma"], _scalar(dtype), _dyn_info(nx, nu, dtype, "default"))


@pytest.mark.parametrize("engine", [e for e in DYN_ENV if e != "default"])
@pytest.mark.parametrize("nx,nu", [(5, 3), (17, 5), (33, 7), (16, 16), (48, 32), (64, 32)],
                         ids=["5x3", "17x5", "33x7", "16x16", "48x32", "64x32"])
def test_dynamics_engines(nx, nu, engine):
    """fp64 (an fp32 context always runs k_d2_*<float>, which every fp32 case above covers): the
    per-stage fallback, the split sweep where the plan admits it ((33, 7); elsewhere kernel_info
    reports the tier launches it falls back to, asserted), the tier launches and the per-stage
    MFMA tiles, on three odd and three even shapes."""
    _check_case(bc.shape_tree(nx, nu), nx, nu, "float64", DYN_ENV[engine], _scalar("float64"),
                _dyn_info(nx, nu, "float64", engine))


@pytest.mark.parametrize("nx,nu", [(65, 32), (64, 33), (65, 33)])
def test_sizes_beyond_the_tiles_are_refused(nx, nu):
    """nx = 65 or nu = 33 has no MFMA instantiation: raocp_ctx_create refuses it with the argument
    error (RAOCP_ERR_ARG, -1) in validate_tree, before any HIP call, so nothing was allocated or
    launched; a context of an admitted size works afterwards."""
    P, v = np.full((2, 2), .5), np.full(2, .5)
    prob = build_problem(recipe_general(P, v, 2, 2, nx, nu, seed=1))[1]
    with pytest.raises(RaocpError, match=r"error -1: the CP kernels support nx <= 64 and nu <= 32"):
        core.Cache(prob)
    ok = core.Cache(bc.problem(bc.shape_tree(1, 1))[1])
    assert ok.native.kernel_info(10) == _scalar("float64")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nx,nu", [(5, 3), (17, 5)], ids=["5x3", "17x5"])
def test_batch_and_mpc(nx, nu, dtype, monkeypatch):
    """Solver.chock_batch with B = 3 against three sequential chock solves of the same context type
    (fp64: 1e-8 per trace entry, 1e-9 on the iterate, test_gpu_batch.py; fp32: 1e-4 and 1e-5,
    test_gpu_batch_fp32.py) and against the oracle in fp64; simulate_batch with 2 steps
    replayed bit for bit by chock_batch from the recorded states, and its plant step
    (test_gpu_mpc.py). k_cpb and k_mpc_step by name: dense tables per mode, staged in LDS."""
    f32 = dtype == "float32"
    if f32:
        monkeypatch.setenv("RAOCP_CPB_F32", "1")
    tree = bc.shape_tree(nx, nu)
    r, prob, op, alpha = bc.problem(tree)
    tol_t, tol_z = (1e-4, 1e-5) if f32 else (1e-8, 1e-9)
    s = core.Solver(problem_spec=prob, dtype=dtype)
    nat = s.cache.native
    assert nat.kernel_info(13) == ("k_cpb<float, true>" if f32 else "k_cpb<true>")
    assert nat.kernel_info(14) == ("k_mpc_step<float>" if f32 else "k_mpc_step")
    x0 = np.asarray(r["x0"], dtype=float).reshape(-1)
    X = np.stack([x0, 0.5 * x0, 0.1 * x0])
    K = 19
    status = s.chock_batch(X, max_iters=K, tol=0.0, step_size=alpha)
    for b in range(3):
        one = core.Solver(problem_spec=prob, dtype=dtype)
        assert one.chock(X[b].reshape(-1, 1), max_iters=K, tol=0.0, step_size=alpha) == int(status[b]) == 1
        figs = (trace_rel_err(s.batch_error_cache[b], one.error_cache), trace_rel_err(s.batch_delta_error_cache[b], one.delta_error_cache),
                rel_err(s.batch_primal_flat(b), one.cache.get_primal_flat()), rel_err(s.batch_dual_flat(b), one.cache.get_dual_flat()))
        print(f"shapes batch {tree} {dtype} instance {b} vs sequential: traces {figs[0]:.2e} / {figs[1]:.2e} iterate {figs[2]:.2e} / {figs[3]:.2e}")
        assert figs[0] <= tol_t and figs[1] <= tol_t and figs[2] <= tol_z and figs[3] <= tol_z, figs
        if not f32:
            st_o, err_o, derr_o, z_o, e_o, _ = op.chock(X[b], K, 0.0, alpha=alpha)
            assert trace_rel_err(s.batch_error_cache[b], err_o) <= 1e-8 and rel_err(s.batch_primal_flat(b), z_o) <= 1e-9
    # closed loop: 2 steps, every root child on some path
    nc = len(prob.tree.children_of(0))
    scen = np.array([[(b + t) % nc for t in range(2)] for b in range(3)], dtype=np.int64)
    res = s.simulate_batch(X, 2, scenarios=scen, max_iters=K, tol=0.0, step_size=alpha, warm=True)
    rep = core.Solver(problem_spec=prob, dtype=dtype)
    for t in range(2):
        st = rep.chock_batch(res.states[:, t], max_iters=K, tol=0.0, step_size=alpha, warm=t > 0)
        assert np.array_equal(res.status[:, t], st)
        assert np.array_equal(res.errors[:, t], np.stack([np.atleast_2d(rep.batch_error_cache[b])[-1] for b in range(3)]))
        assert np.array_equal(res.inputs[:, t], rep.batch_first_inputs())
        for b in range(3):
            i = int(prob.tree.children_of(0)[scen[b, t]])
            A, Bm = (np.asarray(m, dtype=np.float32 if f32 else float).astype(float)
                     for m in (prob.state_dynamics_at_node(i), prob.control_dynamics_at_node(i)))
            x, u = res.states[b, t], res.inputs[b, t]
            bound = (nx + nu + 1) * (2.0 ** -23 if f32 else 2.0 ** -52) * (np.abs(A) @ np.abs(x) + np.abs(Bm) @ np.abs(u))
            assert np.all(np.abs(res.states[b, t + 1] - (A @ x + Bm @ u)) <= bound), (b, t)
    for b in range(3):
        assert np.array_equal(s.batch_primal_flat(b), rep.batch_primal_flat(b))
