"""The trees and crafted warm starts shared by tests/test_branch_census.py (CPU: the oracle's
census of every start) and tests/test_gpu_branches.py (GPU: every CP kernel family on them).

A cold-started CP trajectory on the suite's trees stays in the scaling branch of the
second-order-cone projection and almost wholly inside the boxes ("Branch coverage of
the dual step"), so these starts are built to take every branch in their first iteration
(helpers.crafted_start) and the census test proves that they do.
"""
import functools
import os

import numpy as np

from raocp.problems import build_problem, recipe_from_npz, recipe_general, recipe_general_small, recipe_synthetic
from helpers import crafted_rotations, crafted_start

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GOLDEN_FILE = {"main": "main_trace", "bin6": "traj_small", "c1n5": "traj_small"}
# Seeds of the crafted starts: the smallest for which the start meets every census condition
# (census_violations; tests/test_branch_census.py asserts them for every start used). The
# synthetic trees all take 1; the small cones of main (nx = 3) and c1n5 (nx = 4) leave a cone
# kept at its random value near an edge more often, so fewer seeds qualify there.
# The "-dense" trees have boxes of their own (a bound per entry, some one-sided), so a tree's
# name is looked up before its base.
SEED = 1
SEEDS = {"main": 32, "c1n5": 5,
         # the shape sweep's small cones (nx = 1, 5, 6): the smallest seed that qualifies
         "s1x1": 82, "s1x1u": 82, "s5x3": 3, "s5x3u": 3, "s6x18": 3, "s6x18u": 3,
         # the wide trees (5 / 3: cones of 6 to 9 entries, 280 to 600 of them on w5 and w17)
         "w5": 110, "w5u": 163, "w17": 207, "w17u": 2700, "r12": 2, "r12u": 2, "w64r": 3, "w64ru": 6,
         "w65r": 4, "w65ru": 4, "w82r": 2, "w82ru": 2}
# one start per instance of a batch
BATCH_SEEDS = {"main": (32, 37, 50), "bin6": (1, 2, 3), "c1n5": (5, 12, 46), "m7x32": (1, 2, 3),
               "m7x32-dense": (1, 2, 3)}
# the wide trees' batch starts: three seeds where one start covers the tree, one
# seed whose three rotations are the three instances where it takes the three (ROTATIONS)
WIDE_BATCH_SEEDS = {"w5": (110, 163, 183), "w17": (207, 953, 1162), "r12": (2,), "w65r": (4,)}
# the form of the batch kernel each problem reaches (kernel_info(13)), fp64 / fp32: the tables of the
# golden problems fit the kernel's LDS budget and are staged there, those of m7x32 are read from HBM
BATCH_KERNEL = {"main": ("k_cpb<true>", "k_cpb<float, true>"), "bin6": ("k_cpb<true>", "k_cpb<float, true>"),
                "c1n5": ("k_cpb<true>", "k_cpb<float, true>"), "m7x32": ("k_cpb<false>", "k_cpb<float, false>"),
                "m7x32-dense": ("k_cpb<false>", "k_cpb<float, false>")}
# the form of the accelerated batch kernel (kernel_info(19), fp64 only) on the trees of
# tests/accel_cases.py: the same rule, so only the 75 KB of m7x32's tables are read from HBM
CPA_KERNEL = {"main": "k_cpa<true>", "s1x1": "k_cpa<true>", "s5x3": "k_cpa<true>", "s17x5": "k_cpa<true>",
              "s16x16": "k_cpa<true>", "g53": "k_cpa<true>", "m7x32": "k_cpa<false>", "m7x32-dense": "k_cpa<false>"}
ENTRY_SEEDS = {"bin7": 1, "main": 22}  # the stand-alone entry points project the crafted dual itself
T_OFFSET = 50.0
ITERS = (0, 2)  # max_iters of the two runs of every case: one iteration, three iterations


def _uniform(C):
    return np.full((C, C), 1.0 / C), np.full(C, 1.0 / C)


def _synthetic(C, N, nx, nu, seed):
    P, v = _uniform(C)
    return recipe_synthetic(P, v, N, N, nx, nu, seed=seed)


def _seven_modes():
    """31 nodes, binary branching, 7 Markov modes (each with two successors) at 32 / 12 with a cost
    per mode: 7 sqrtQ and 7 sqrtR tables, 37 KB in float and 75 KB in double, beyond the 32 KiB of
    LDS the batch kernel stages its tables in, so it reaches k_cpb<false> and k_cpb<float, false>
    (every mode must occur for its table to be packed, which takes 4 stages from 2 initial modes)."""
    M = 7
    P = np.zeros((M, M))
    for i in range(M):
        P[i, i] = P[i, (i + 1) % M] = 0.5
    v = np.zeros(M)
    v[0] = v[3] = 0.5
    r = recipe_synthetic(P, v, 4, 4, 32, 12, seed=9)
    r["Q"] = np.array([(1.0 + k) * q for k, q in enumerate(r["Q"])])
    r["R"] = np.array([(2.0 + k) * q for k, q in enumerate(r["R"])])
    return r


def _dense(base, r):
    """The tree, A, B and x0 of r with the weights and boxes of recipe_general: dense sqrtQ, sqrtR and
    sqrtPf tables, a bound of its own per box entry, every eighth entry one-sided. Where the plain
    tree has one cost over all modes so has this one (the streaming L / L^T and the fused CP
    kernels take one weight table per tree; with a table per mode the library would, rightly, run
    other kernels than the plain sibling's); where it has a cost per mode (m7x32) the dense
    tables differ per mode too."""
    shared = len({q.tobytes() for q in r["Q"]}) == 1 and len({q.tobytes() for q in r["R"]}) == 1
    g = recipe_general(r["P"], r["v"], r["N"], r["tau"], r["A"].shape[1], r["B"].shape[2],
                       seed=sum(map(ord, base)), alpha_r=r["alpha_r"], shared_weights=shared)
    for k in ("Q", "R", "Pf", "nl_min", "nl_max", "l_min", "l_max"):
        r[k] = g[k]
    return r


# name -> recipe; "-nobox" drops every box, "-leafbox" the nonleaf ones, "-dense": _dense
_TREES = {
    "bin3": lambda: _synthetic(2, 3, 20, 8, 11),       # 15 nodes
    "bin4": lambda: _synthetic(2, 4, 20, 8, 22),       # 31 nodes
    "bin7": lambda: _synthetic(2, 7, 20, 8, 12),       # 255 nodes
    "bin8": lambda: _synthetic(2, 8, 20, 8, 21),       # 511 nodes
    "chain12": lambda: _synthetic(1, 12, 20, 8, 3),    # 13 nodes, one leaf
    "bin32d5": lambda: _synthetic(2, 5, 32, 12, 4),    # 63 nodes
    "quad20d4": lambda: _synthetic(4, 4, 20, 8, 6),    # 341 nodes
    "tern32d4": lambda: _synthetic(3, 4, 32, 12, 4),   # 121 nodes
    "quad64d3": lambda: _synthetic(4, 3, 64, 16, 7),   # 85 nodes
    "m7x32": _seven_modes,                             # 31 nodes, tables beyond the batch kernel's LDS
    "g53": lambda: recipe_general_small("g53"),        # 27 nodes, 1 / 2 / 3 children, 5 / 3
}


# ---- the shape sweep (tests/test_gpu_shapes.py): (nx, nu) -> branching, horizon and risk level of
# its tree, 31 (binary, N = 4), 40 (ternary, N = 3) or 121 (ternary, N = 4) nodes, so that one
# crafted start reaches every cone class on 30 % of the cones (helpers.crafted_rotations). Each shape
# has two trees of recipe_general: "s<nx>x<nu>" with dense weight tables per mode (the node blocks
# mix tables) and "s<nx>x<nu>u" with one dense table over the modes, which the MFMA CP kernels need.
SHAPES = {(1, 1): (2, 4, 0.1), (5, 3): (3, 3, 0.7), (6, 18): (2, 4, 0.99), (16, 16): (2, 4, 0.1), (17, 5): (3, 3, 0.7),
          (24, 17): (2, 4, 0.99), (33, 7): (3, 3, 0.1), (48, 32): (2, 4, 0.7), (49, 9): (3, 4, 0.99), (64, 32): (2, 4, 0.1)}


def shape_tree(nx, nu, shared=False):
    return f"s{nx}x{nu}" + ("u" if shared else "")


def _shape_recipe(nx, nu, shared):
    C, N, alpha_r = SHAPES[(nx, nu)]
    P, v = _uniform(C)
    return recipe_general(P, v, N, N, nx, nu, seed=100 * nx + nu, alpha_r=alpha_r, shared_weights=shared)


for _nx, _nu in SHAPES:
    for _sh in (False, True):
        _TREES[shape_tree(_nx, _nu, _sh)] = functools.partial(_shape_recipe, _nx, _nu, _sh)
SHAPE_TREES = tuple(shape_tree(nx, nu, sh) for nx, nu in SHAPES for sh in (False, True))


# ---- wide branching: 5 to 82 children per node, where no `<= 4` fast path
# applies and the lane groups sized by cmax span one to several waves. name -> (modes, kind, N, nx,
# nu, alpha_r): "full": v uniform, P uniform and full (every node has `modes` children); "ragged": v
# uniform, row i of P has 1 + (7 i mod modes) successors i, i + 1, .. with random weights (1 .. 12
# children at 12 modes); "root": v uniform, P[i] = 1/2 on i and i + 1 (a wide root over binary stages).
# Each has two trees of recipe_general like the shape sweep: a dense weight table per mode, and "<name>u"
# with one table over the modes. w83r is one past the admitted maximum (check_group: 257 lanes).
# CPU only so far (the census of their starts, the oracle's golden pins): raocp_ctx_create does not survive a
# root of five or more children, so no GPU test creates a context on them yet.
_WIDE = {"w5": (5, "full", 3, 5, 3, 0.1), "w8": (8, "full", 2, 20, 8, 0.7), "w17": (17, "full", 2, 5, 3, 0.99),
         "r12": (12, "ragged", 2, 17, 5, 0.1), "w64r": (64, "root", 2, 5, 3, 0.7), "w65r": (65, "root", 2, 5, 3, 0.99),
         "w82r": (82, "root", 2, 5, 3, 0.1), "w8s": (8, "full", 2, 5, 3, 0.7), "w83r": (83, "root", 2, 5, 3, 0.1)}
WIDE = ("w5", "w8", "w17", "r12", "w64r", "w65r", "w82r")
WIDE_NODES = {"w5": 156, "w8": 73, "w17": 307, "r12": 91, "w64r": 193, "w65r": 196, "w82r": 247}


def wide_chain(M, kind, seed):
    """(P, v) of a wide tree's Markov chain (see _WIDE)."""
    v = np.full(M, 1.0 / M)
    if kind == "full":
        return np.full((M, M), 1.0 / M), v
    P = np.zeros((M, M))
    if kind == "root":
        for i in range(M):
            P[i, i] = P[i, (i + 1) % M] = 0.5
        return P, v
    assert kind == "ragged", kind
    rng = np.random.default_rng([seed, 2])
    for i in range(M):
        k = 1 + (7 * i) % M
        w = rng.uniform(0.5, 1.5, k)
        P[i, (i + np.arange(k)) % M] = w / w.sum()
    return P, v


def _wide_recipe(name, shared):
    M, kind, N, nx, nu, alpha_r = _WIDE[name]
    seed = 1000 + sum(map(ord, name))
    P, v = wide_chain(M, kind, seed)
    return recipe_general(P, v, N, N, nx, nu, seed=seed, alpha_r=alpha_r, shared_weights=shared)


for _name in _WIDE:
    for _sh in (False, True):
        _TREES[_name + ("u" if _sh else "")] = functools.partial(_wide_recipe, _name, _sh)
WIDE_TREES = tuple(t + s for t in WIDE for s in ("", "u"))


@functools.lru_cache(maxsize=None)
def problem(tree):
    """(recipe, RAOCP problem, OracleProblem, alpha) of a tree, built once. alpha: the golden
    fixtures' pinned step size, else the oracle's own (0.999 / lambda_max by ARPACK)."""
    from oracle.raocp_oracle import OracleProblem
    base, _, variant = tree.partition("-")
    if base in GOLDEN_FILE:
        z = np.load(os.path.join(GOLDEN, GOLDEN_FILE[base] + ".npz"))
        r = recipe_from_npz(z, base)
        alpha = float(z[f"{base}/cp_alpha"])
    else:
        r = _TREES[base]()
        alpha = None
    if variant == "dense":
        assert base in _TREES, tree
        r = _dense(base, r)
    elif variant in ("nobox", "leafbox"):
        r["nl_min"] = r["nl_max"] = None
        if variant == "nobox":
            r["l_min"] = r["l_max"] = None
    else:
        assert variant == "", tree
    _, prob = build_problem(r)
    op = OracleProblem(prob)
    if alpha is None:
        alpha = op.step_size()[1]
    return r, prob, op, alpha


def seed_of(tree):
    return SEEDS.get(tree, SEEDS.get(tree.partition("-")[0], SEED))


# The wide root of w64r / w65r / w82r is the only parent with a child slot >= 2, and slot 11 of r12
# has two parents: one start gives such a slot one class, so these take the three rotated starts (every
# cone takes each class once), like the trees too small for the 30 % shares.
ROTATIONS = {t + s: 3 for t in ("r12", "w64r", "w65r", "w82r") for s in ("", "u")}


# their 250 to 400 cones of 6 to 9 entries: see helpers.crafted_start
CALM = frozenset(ROTATIONS) - {"r12", "r12u"}


def rotations(tree):
    return ROTATIONS.get(tree, crafted_rotations(problem(tree)[2]))


@functools.lru_cache(maxsize=None)
def start(tree, rot, seed, f32=False):
    """(p0, d0, child classes, leaf classes) of the tree's crafted start, read-only. f32: the
    start rounded to float, which is what a float context holds after set_primal / set_dual."""
    r, prob, op, alpha = problem(tree)
    p0, d0, ccls, lcls = crafted_start(op, alpha, seed, T_OFFSET, rot, calm=tree in CALM)
    if f32:
        p0, d0 = p0.astype(np.float32).astype(np.float64), d0.astype(np.float32).astype(np.float64)
    for a in (p0, d0, ccls, lcls):
        a.setflags(write=False)
    return p0, d0, ccls, lcls


@functools.lru_cache(maxsize=None)
def reference(tree, K, rot, seed, f32=False, x0_scale=1.0):
    """OracleProblem.chock(x0_scale * x0, K, 0.0, alpha, p0, d0) from the crafted start: (status,
    err, derr, z, eta), computed once and read-only."""
    r, prob, op, alpha = problem(tree)
    p0, d0, _, _ = start(tree, rot, seed, f32)
    x0 = x0_scale * np.asarray(r["x0"], dtype=float).reshape(-1)
    st, err, derr, z, e, _ = op.chock(x0, K, 0.0, alpha=alpha, p0=p0, d0=d0)
    for a in (err, derr, z, e):
        a.setflags(write=False)
    return st, err, derr, z, e


@functools.lru_cache(maxsize=None)
def modified_dual(tree, rot, seed):
    """The modified dual iteration 1 projects from the crafted start (read-only)."""
    r, prob, op, alpha = problem(tree)
    p0, d0, _, _ = start(tree, rot, seed)
    v = op.chock_modified_duals(r["x0"], 0, alpha, p0=p0, d0=d0)[0]
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def census(tree, rot, seed):
    """The oracle's branch census of iteration 1 from the crafted start."""
    return problem(tree)[2].branch_census(modified_dual(tree, rot, seed))


# golden main's leaf box is +-7 on a state of order 1: a standard normal start cannot reach its lo
# or hi branch (its nonleaf box, +-0.1 on the inputs, is left on both sides). The leaf-box sites of
# the kernels main runs (scalar, batch) are reached on bin7, bin6 and c1n5.
BOX_EXEMPT = {"main": ("box_l",)}


def box_exempt(tree):
    return BOX_EXEMPT.get(tree.partition("-")[0], ())


def census_violations(op, cens, exempt=()):
    """The conditions a crafted start must meet in iteration 1, checked on the census of each of
    its rotations (cens); returns the list of those it misses (empty: a valid start).
      - each SOC class on >= 30 % of the child cones and of the leaf cones (over the rotations);
      - every margin >= 0.1;
      - every (child slot within its parent, class) pair;
      - each box branch on >= 5 % of the boxed entries, for the nonleaf boxes (eta7) and the leaf
        boxes (eta14) separately, since they are separate code in every kernel (exempt: the kinds
        of BOX_EXEMPT, which the caller names);
      - each sign on >= 10 % of the clamped eta1 and eta2 entries."""
    bad = []
    for kind in ("child", "leaf"):
        cls = np.concatenate([c[kind + "_class"] for c in cens])
        share = np.bincount(cls, minlength=3) / cls.size
        if share.min() < 0.30:
            bad.append(f"{kind} cone classes {np.round(share, 3).tolist()} < 30 %")
        mar = min(float(c[kind + "_margin"].min()) for c in cens)
        if mar < 0.1:
            bad.append(f"{kind} cone margin {mar:.3g} < 0.1")
    rank = op.rank[op.kids]
    pairs = {(int(s), int(k)) for c in cens for s, k in zip(rank, c["child_class"])}
    missing = {(s, k) for s in range(int(op.nch.max())) for k in range(3)} - pairs
    if missing:
        bad.append(f"(child slot, class) pairs missing: {sorted(missing)}")
    for q, c in enumerate(cens):
        for key in ("box_nl", "box_l"):
            box = c[key]
            if key not in exempt and box.sum() and box.min() < 0.05 * box.sum():
                bad.append(f"start {q}: {key} lo / hi / inside {box.tolist()} < 5 %")
        for key, total in (("eta1_sign", op.y_all.size - op.m), ("eta2_sign", op.m)):
            if c[key].min() < 0.10 * total:
                bad.append(f"start {q}: {key} + / - {c[key].tolist()} of {total} < 10 %")
    return bad


TIE_TREES = ("bin7", "main", "chain12")


@functools.lru_cache(maxsize=None)
def tie_dual(tree, seed=9):
    """A dual on the edges of the projections' comparisons. Five kinds of cone in turn over the
    child cones and over the leaf cones: F = 0 with t = 2, t = 0, t = -2; nf == t and nf == -t
    held exactly (F = (3, 0, .., 0, 4) with the 4 in the cone's last F entry, eta5 / eta12, so
    that the norm spans its segments; 9 + 16 = 25 is exact in any summation order and in either
    precision; t = 5, -5). Of every box row, one entry in three sits exactly at lo and the next
    exactly at hi. Returns (v, child cone entry indices [cones, F.. t], which child cones the
    projection must return unchanged (the others it must zero), and the same two for the leaf cones)."""
    r, prob, op, alpha = problem(tree)
    nx, nu = op.nx, op.nu
    rng = np.random.default_rng(seed)
    v = np.where(op.live_masks()[1], rng.standard_normal(op.D), 0.0)
    j, lf = op.kids, op.leaves
    child = np.concatenate([op.E3[j][:, None] + np.arange(nx), op.E4[j][:, None] + np.arange(nu),
                            op.E5[j][:, None], op.E6[j][:, None]], axis=1)
    leaf = np.concatenate([op.E11[lf][:, None] + np.arange(nx), op.E12[lf][:, None], op.E13[lf][:, None]], axis=1)
    keeps = []
    for idx in (child, leaf):
        kind = np.arange(idx.shape[0]) % 5
        v[idx[:, :-1]] = 0.0
        v[idx[kind >= 3, 0]] = 3.0
        v[idx[kind >= 3, -2]] = 4.0
        v[idx[:, -1]] = np.array([2.0, 0.0, -2.0, 5.0, -5.0])[kind]
        keeps.append(np.isin(kind, (0, 1, 3)))
    act, lact = np.flatnonzero(op.nl_active), np.flatnonzero(op.l_active)
    for idx, lo, hi in ((op.E7[act][:, None] + np.arange(nx + nu), op.nl_lo[act], op.nl_hi[act]),
                        (op.E14[lf[lact]][:, None] + np.arange(nx), op.l_lo[lact], op.l_hi[lact])):
        if idx.size:
            col = np.arange(idx.shape[1])[None, :] + np.arange(idx.shape[0])[:, None]
            v[idx] = np.where(col % 3 == 0, lo, np.where(col % 3 == 1, hi, v[idx]))
    v.setflags(write=False)
    return v, child, keeps[0], leaf, keeps[1]


# ---- the kernel families (tests/test_gpu_branches.py). A case: id, tree, the environment its
# context is created under (as the family's own test file selects it), dtype, and what
# kernel_info must report: (op, "eq" | "starts", text).
_DRC = [(11, "eq", "k_drc<20, 8, 2>")]
_CP6 = [(11, "eq", ""), (9, "eq", "k_dr<20, 8> x1"), (10, "eq", "k_cp6<double, 20, 8, 2>")]
_CP4 = [(11, "eq", ""), (10, "eq", "k_cp4<double, 20, 8>")]
_CP3_20 = [(11, "eq", ""), (10, "starts", "k_cp3<double, 20, 8")]
_NO6, _NO4 = {"RAOCP_DRC": "0", "RAOCP_CP6": "0"}, {"RAOCP_DRC": "0", "RAOCP_CP6": "0", "RAOCP_CP4": "0"}
_MFMA = {"RAOCP_CP3": "0", "RAOCP_CP_V1": "0"}
_SCALAR = {"RAOCP_CP3": "0", "RAOCP_CP_V1": "1"}

FAMILIES = [
    ("drc-bin4", "bin4", {"RAOCP_DR_CUTS": ""}, "float64", _DRC),
    ("drc-bin4-nobox", "bin4-nobox", {"RAOCP_DR_CUTS": ""}, "float64", _DRC),
    ("drc-bin8", "bin8", {"RAOCP_DR_CUTS": "4"}, "float64", _DRC),
    ("drc-bin8-nobox", "bin8-nobox", {"RAOCP_DR_CUTS": "4"}, "float64", _DRC),
    ("cp6-bin3", "bin3", {"RAOCP_DRC": "0"}, "float64", _CP6),
    ("cp6-bin3-nobox", "bin3-nobox", {"RAOCP_DRC": "0"}, "float64", _CP6),
    ("cp6-bin7", "bin7", {"RAOCP_DRC": "0"}, "float64", _CP6),
    ("cp6-bin7-nobox", "bin7-nobox", {"RAOCP_DRC": "0"}, "float64", _CP6),
    ("cp6-bin4", "bin4", {"RAOCP_DRC": "0", "RAOCP_DR_CUTS": ""}, "float64", _CP6),
    ("cp6-bin8", "bin8", {"RAOCP_DRC": "0", "RAOCP_DR_CUTS": "4"}, "float64", _CP6),
    ("cp4-bin7", "bin7", _NO6, "float64", _CP4),
    ("cp4-bin7-leafbox", "bin7-leafbox", _NO6, "float64", _CP4),
    ("cp4-bin8", "bin8", dict(_NO6, RAOCP_DR_CUTS="4"), "float64", _CP4),
    ("cp3-bin7-split1", "bin7", dict(_NO4, RAOCP_CP3_SPLIT="1"), "float64", _CP3_20),
    ("cp3-bin7-split0", "bin7", dict(_NO4, RAOCP_CP3_SPLIT="0"), "float64", _CP3_20),
    ("cp3-bin8", "bin8", dict(_NO4, RAOCP_DR_CUTS="4"), "float64", _CP3_20),
    ("cp3-chain12", "chain12", {}, "float64", _CP3_20),
    ("cp3-bin32d5", "bin32d5", {}, "float64", [(10, "starts", "k_cp3<double, 32, 12")]),
    ("mfma-bin7", "bin7", _MFMA, "float64", [(10, "eq", "k_cpd2<double, 2, 1> + k_cpp2<double, 2, 1>")]),
    ("scalar-bin7", "bin7", _SCALAR, "float64", [(10, "eq", "k_cpd<double, 20, 8> + k_cpp<double, 20, 8>")]),
    ("scalar-main", "main", _SCALAR, "float64", [(10, "eq", "k_cpd<double, 3, 2> + k_cpp<double, 3, 2>")]),
    ("cp5-quad20d4", "quad20d4", {}, "float64", [(10, "starts", "k_cp5_leaf<double, 20, 4> x1 + k_cp5_fams<double, 20, 8, 4>")]),
    ("cp5-tern32d4", "tern32d4", {}, "float64", [(10, "starts", "k_cp5_leaf<double, 32, 3> x1 + k_cp5_fams<double, 32, 12, 3>")]),
    ("cp3-quad20d4", "quad20d4", {"RAOCP_CP5": "0"}, "float64", _CP3_20[1:]),
    ("cp3-tern32d4", "tern32d4", {"RAOCP_CP5": "0"}, "float64", [(10, "starts", "k_cp3<double, 32, 12")]),
    ("f32-cp5-quad64d3", "quad64d3", {}, "float32", [(10, "starts", "k_cp5_leaf<float, 64, 4> x1 + k_cp5_fams<float, 64, 16, 4>")]),
    ("f32-cp3-quad64d3", "quad64d3", {"RAOCP_CP5": "0"}, "float32", [(10, "starts", "k_cp3<float, 64, 16")]),
    ("f32-cp3-bin7", "bin7", {}, "float32", [(10, "starts", "k_cp3<float, 20, 8")]),
]
# the same kernels on the "-dense" tree of the same name: each keeps its plain sibling's
# environment, dtype and kernel_info strings
DENSE = ("drc-bin4", "drc-bin8", "cp6-bin7", "cp4-bin7", "cp3-bin7-split1", "cp3-bin32d5", "mfma-bin7", "scalar-bin7",
         "cp5-quad20d4", "cp5-tern32d4", "f32-cp5-quad64d3", "f32-cp3-bin7")
FAMILIES += [(c[0] + "-dense", c[1] + "-dense") + c[2:] for c in FAMILIES if c[0] in DENSE]
assert len(FAMILIES) == 28 + len(DENSE)
FAMILY = {c[0]: c for c in FAMILIES}

# kernels that claim to share arithmetic, and the bound the suite already holds them to
AGREE = [
    ("drc-bin8", "cp6-bin8", 1e-12), ("cp6-bin8", "cp4-bin8", 1e-12), ("cp6-bin8", "cp3-bin8", 1e-12),
    ("drc-bin4", "cp6-bin4", 1e-12),
    ("cp6-bin7", "cp4-bin7", 1e-12), ("cp6-bin7", "cp3-bin7-split1", 1e-12), ("cp3-bin7-split1", "cp3-bin7-split0", 1e-12),
    ("cp5-quad20d4", "cp3-quad20d4", 1e-12), ("cp5-tern32d4", "cp3-tern32d4", 1e-12),
    ("mfma-bin7", "cp3-bin7-split1", 1e-10),
    ("cp6-bin7-dense", "cp4-bin7-dense", 1e-12), ("cp6-bin7-dense", "cp3-bin7-split1-dense", 1e-12),
    ("mfma-bin7-dense", "cp3-bin7-split1-dense", 1e-10),
]

BATCH_TREES = tuple(BATCH_SEEDS)
ENTRY_TREES = tuple(ENTRY_SEEDS)


# ---- the sharded path (tests/test_gpu_shard_branches.py). A case: id, tree, the environment its
# contexts are created under, dtype, what kernel_info must report for every shard ((op, "eq" |
# "starts" | "has", text)), how raocp_shard_setup picks the cut stage ("tiers": the tier planner's
# cut; "dyn3": the first stage with >= 8 R nodes) and the shard counts R: every one of 1 (under
# RAOCP_SHARD_FORCE=1), 2, 3, 4, 8 that shard setup accepts on the tree. The tiered sweep cuts bin8
# at stage 4 (16 roots: every R; R = 3 owns 5 / 5 / 6) and s64x32 at stage 1 (2 roots: R <= 2);
# the per-stage sweep needs a stage before the leaves with 8 R nodes: quad20d4 (1, 4, 16, 64, 256)
# every R, tern32d4 (1, 3, 9, 27, 81) R <= 3, quad64d3 (1, 4, 16, 64) R <= 2.
_SH_PINS = {"RAOCP_DR": "0", "RAOCP_CP4": "0", "RAOCP_CP5": "0", "RAOCP_CP6": "0"}  # test_gpu_shard.py _kern_cache
_TIERS_20 = (9, "has", "k_dyn_bottom_back<20, 8")
_SH_CP3 = [_TIERS_20, (10, "eq", "k_cp3<double, 20, 8, true> x2")]
_SH_MFMA = [_TIERS_20, (10, "eq", "k_cpd2<double, 2, 1> + k_cpp2<double, 2, 1>")]
_DY3 = "k_dy3_top_back"
SHARDED = [
    ("sh-cp3-bin8", "bin8", _SH_PINS, "float64", _SH_CP3, "tiers", (1, 2, 3, 4, 8)),
    ("sh-cp3-bin8-dense", "bin8-dense", _SH_PINS, "float64", _SH_CP3, "tiers", (1, 2, 3, 4, 8)),
    ("sh-mfma-bin8", "bin8", dict(_SH_PINS, **_MFMA), "float64", _SH_MFMA, "tiers", (1, 2, 3, 4, 8)),
    ("sh-mfma-bin8-dense", "bin8-dense", dict(_SH_PINS, **_MFMA), "float64", _SH_MFMA, "tiers", (1, 2, 3, 4, 8)),
    # a table per mode: the node blocks of the scalar kernels mix tables (the MFMA ones need one table)
    ("sh-scalar-s64x32", "s64x32", dict(_SH_PINS, RAOCP_CP3="0"), "float64",
     [(9, "has", "k_dyn_bottom_back<0, 0"), (10, "eq", "k_cpd<double, 0, 0> + k_cpp<double, 0, 0>")], "tiers", (1, 2)),
    ("sh-cp5-quad20d4", "quad20d4", {"RAOCP_DYN3": "1"}, "float64",
     [(9, "has", _DY3), (10, "starts", "k_cp5_leaf<double, 20, 4> x1 + k_cp5_fams<double, 20, 8, 4>"), (10, "has", "after X1")],
     "dyn3", (1, 2, 3, 4, 8)),
    ("sh-cp5-quad20d4-dense", "quad20d4-dense", {"RAOCP_DYN3": "1"}, "float64",
     [(9, "has", _DY3), (10, "starts", "k_cp5_leaf<double, 20, 4> x1 + k_cp5_fams<double, 20, 8, 4>"), (10, "has", "after X1")],
     "dyn3", (1, 2, 3, 4, 8)),
    ("sh-cp5-tern32d4", "tern32d4", {"RAOCP_DYN3": "1"}, "float64",
     [(9, "has", _DY3), (10, "starts", "k_cp5_leaf<double, 32, 3> x1 + k_cp5_fams<double, 32, 12, 3>"), (10, "has", "after X1")],
     "dyn3", (1, 2, 3)),
    ("sh-cp5-tern32d4-dense", "tern32d4-dense", {"RAOCP_DYN3": "1"}, "float64",
     [(9, "has", _DY3), (10, "starts", "k_cp5_leaf<double, 32, 3> x1 + k_cp5_fams<double, 32, 12, 3>"), (10, "has", "after X1")],
     "dyn3", (1, 2, 3)),
    ("sh-f32-cp5-quad64d3", "quad64d3", {}, "float32",
     [(9, "has", _DY3), (10, "starts", "k_cp5_leaf<float, 64, 4> x1 + k_cp5_fams<float, 64, 16, 4>"), (10, "has", "after X1")],
     "dyn3", (1, 2)),
    ("sh-f32-cp5-quad64d3-dense", "quad64d3-dense", {}, "float32",
     [(9, "has", _DY3), (10, "starts", "k_cp5_leaf<float, 64, 4> x1 + k_cp5_fams<float, 64, 16, 4>"), (10, "has", "after X1")],
     "dyn3", (1, 2)),
    ("sh-f32-cp3-quad64d3", "quad64d3", {"RAOCP_CP5": "0"}, "float32",
     [(9, "has", _DY3), (10, "eq", "k_cp3<float, 64, 16, true> x2")], "dyn3", (1, 2)),
]
SHARDED_CASE = {c[0]: c for c in SHARDED}
SHARD_TREES = tuple(sorted({c[1] for c in SHARDED}))
# Seeds of the sharded cases' crafted starts: the smallest that meets census_violations and
# cut_census_violations at every cut stage the tree's cases use; the tree's own seed where that does.
# bin8 (seed 1): the owned slices [10, 16) of R = 3 and [12, 16) of R = 4 hold only one sign of the
# roots' eta2; s64x32 (seed 1): the four child cones of its two roots miss the zero class.
SHARD_SEEDS = {"bin8": 5, "bin8-dense": 5, "s64x32": 7}


def shard_seed_of(tree):
    return SHARD_SEEDS.get(tree, seed_of(tree))


N_CUS = 256  # the compute units the tier planner costs its plan for (MI355X)


@functools.lru_cache(maxsize=None)
def tier_cut(tree):
    """The stage raocp_shard_setup cuts a tiered-sweep context of the tree at: c->cut, the tier
    planner's choice, by the planner itself on the host (tests/tierplan/cut_host_main.cpp over
    csrc/raocp_tierplan.h, host compiler) from the tree as raocp_ctx_create hands it over: the
    classes of the packed problem per stage, the (A, B) kinds in order of first use and the (kind,
    parent class) pairs numbered by class (raocp_setup.h, "child kinds" and "number pairs by parent
    class"). 0: the planner found no tier below a top (shard setup refuses the tree)."""
    import shutil
    import subprocess
    import tempfile
    from raocp.core._pack import pack_problem
    pk = pack_problem(problem(tree)[1])
    n, m, N = int(pk.n), int(pk.m), int(pk.N)
    stage_ptr = [int(np.searchsorted(pk.stage, t)) for t in range(N + 1)] + [n]
    kinds, pairs = {}, {}
    for j in range(1, n):
        kid = kinds.setdefault((int(pk.i_a[j]), int(pk.i_b[j])), len(kinds))
        pairs.setdefault((kid, int(pk.i_k[pk.anc[j]])), len(pairs))
    nk = int(pk.n_classes)
    by_class = sorted(c for _, c in pairs)  # the stable sort by parent class keeps the counts per class
    pair_ptr = [int(np.searchsorted(by_class, c)) for c in range(nk)] + [len(pairs)]
    cls_ptr = [int(np.searchsorted(pk.class_stage, t)) for t in range(N + 1)]
    words = [N, n, len(kinds), int(pk.nx), int(pk.nu), N_CUS] + stage_ptr + [m] + [int(v) for v in pk.ch_start[:m]] + \
        [int(v) for v in pk.nch[:m]] + cls_ptr + [nk] + pair_ptr
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "cut_host")
        subprocess.run([cxx, "-std=c++17", "-O1", "-I", os.path.join(root, "raocp-toolbox_amd", "csrc"),
                        os.path.join(root, "tests", "tierplan", "cut_host_main.cpp"), "-o", exe],
                       check=True, capture_output=True, text=True, timeout=300)
        out = subprocess.run([exe], input=" ".join(map(str, words)), check=True, capture_output=True, text=True, timeout=60).stdout
    return int(out.split()[1])


def shard_cut(tree, how, R):
    """The cut stage of R shards of the tree on the host, by raocp_shard_setup's rule: the tier
    planner's cut for the tiered sweep, the first stage before the leaves with >= 8 R nodes for
    the per-stage sweep; None where shard setup refuses (no such stage, or fewer roots than shards)."""
    op = problem(tree)[2]
    width = np.bincount(op.stage)
    if how == "tiers":
        S = tier_cut(tree)
        S = S if 0 < S < op.N else 0
    else:
        S = next((t for t in range(1, op.N) if width[t] >= 8 * R), 0)
    return S if S and width[S] >= R else None


def cut_census_violations(op, vs, S, Rs):
    """The conditions a crafted start must meet at a cut stage S in iteration 1, where the code only
    a shard runs sits (the cut's parents' second CP launch with the roots' eta2 entries from X1; the
    roots' own families, whose eta2 travels), checked on the modified dual of each rotation (vs);
    returns the list of those it misses:
      - every SOC class among the child cones of the stage-S nodes, and among those of their
        children (their leaf cones where the stage-S nodes' children are the leaves);
      - both signs among the pre-clamp eta2 of the stage-S nodes, the entries that travel in X1;
      - both a lo and a hi branch among the eta7 rows of the stage S - 1 parents, where boxed;
      - for each R of Rs, a negative and a positive pre-clamp eta2 in every shard's owned slice of
        stage S of >= 4 nodes (the slice rule of raocp_shard_setup).
    The margins of census_violations (>= 0.1 on every cone of the tree) hold for these cones with it."""
    from helpers import shard_ranges
    bad = []
    cens = [op.branch_census(v) for v in vs]
    kid_stage = op.stage[op.kids]
    groups = [("children of stage S", "child_class", kid_stage == S + 1)]
    if S + 2 <= op.N:
        groups.append(("grandchildren of stage S", "child_class", kid_stage == S + 2))
    else:
        groups.append(("leaf cones below stage S", "leaf_class", op.stage[op.leaves] == S + 1))
    for what, key, sel in groups:
        got = np.bincount(np.concatenate([c[key][sel] for c in cens]), minlength=3)
        if got.min() == 0:
            bad.append(f"S = {S}: cone classes of the {what} {got.tolist()}")
    roots = np.flatnonzero(op.stage == S)
    par = np.flatnonzero((op.stage[:op.m] == S - 1) & op.nl_active)
    for q, v in enumerate(vs):
        e2 = v[op.E2[roots]]
        if not ((e2 > 0).any() and (e2 < 0).any()):
            bad.append(f"S = {S} start {q}: eta2 of the roots has one sign")
        if par.size:
            w = v[op.E7[par][:, None] + np.arange(op.nx + op.nu)]
            lo, hi = (w <= op.nl_lo[par]).sum(), ((w > op.nl_lo[par]) & (w >= op.nl_hi[par])).sum()
            if not (lo and hi):
                bad.append(f"S = {S} start {q}: eta7 of the cut's parents lo / hi {int(lo)} / {int(hi)}")
        for R in Rs:
            for k, (own_lo, own_hi) in enumerate(shard_ranges(op, S, R)):
                e = v[op.E2[own_lo[S]:own_hi[S]]]
                if e.size >= 4 and not ((e > 0).any() and (e < 0).any()):
                    bad.append(f"S = {S} start {q}: eta2 of shard {k} of {R} has one sign")
    return bad


def shard_cuts(tree):
    """{S: the R values cut there} over the sharded cases of a tree."""
    out = {}
    for c in SHARDED:
        if c[1] == tree:
            for R in c[6]:
                out.setdefault(shard_cut(tree, c[5], R), set()).add(R)
    return out

# every (tree, seed) some CP loop on the GPU starts from: the census test covers them all
CENSUS_CASES = sorted({(c[1], seed_of(c[1])) for c in FAMILIES} | {(t, s) for t in BATCH_TREES for s in BATCH_SEEDS[t]} |
                      {(t, seed_of(t)) for t in SHAPE_TREES} | {(t, shard_seed_of(t)) for t in SHARD_TREES} |
                      {(t, seed_of(t)) for t in WIDE_TREES} | {(t, s) for t in WIDE_BATCH_SEEDS for s in WIDE_BATCH_SEEDS[t]})
