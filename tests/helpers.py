"""Shared test helpers (problem construction from golden recipes, comparisons)."""
import numpy as np

from raocp.problems import build_problem, recipe_from_npz


def problem_from_golden(z, name):
    r = recipe_from_npz(z, name)
    tree, prob = build_problem(r)
    return r, tree, prob


def rel_err(a, b):
    a = np.asarray(a, dtype=float)
    b = np.asarray(b, dtype=float)
    scale = max(np.max(np.abs(b)), 1e-300)
    return float(np.max(np.abs(a - b)) / scale) if a.size else 0.0


def balanced_classes(k, rng):
    """k SOC classes (0 identity, 1 zero, 2 scaling), as even as k allows, in a seeded shuffle.
    (Not j % 3: on a ternary tree that gives every child slot one fixed class.)"""
    return rng.permutation(np.arange(k) % 3)


def crafted_rotations(op):
    """How many crafted starts a tree needs for every SOC class to cover >= 30 % of its child
    cones and of its leaf cones: one where a balanced assignment reaches that (floor(k / 3) / k
    >= 0.3 for both kinds), else three with the classes rotated, so that every cone takes each
    class once (a chain has one leaf cone; 14 child cones split 5 / 5 / 4 = 28.6 %)."""
    ok = all(k >= 3 and (k // 3) / k >= 0.3 for k in (op.kids.size, op.leaves.size))
    return 1 if ok else 3


def crafted_start(op, alpha, seed, T=50.0, rot=0):
    """(p0, d0) of a warm start whose first CP iteration takes every branch of the dual step:
    p0 standard normal on the live primal slots, d0 = alpha * standard normal on the live dual
    slots (zero on the placeholders, like every iterate the loop produces); every child cone
    and, by an independent shuffle, every leaf cone gets a class from a balanced seeded
    assignment: identity sets the cone's t entry (eta6 / eta13) of d0 to +alpha T, zero to
    -alpha T, scaling keeps the random value. rot rotates the classes (crafted_rotations).
    Returns (p0, d0, child classes in the order of op.kids, leaf classes in that of op.leaves)."""
    rng = np.random.default_rng(seed)
    pm, dm = op.live_masks()
    p0 = np.where(pm, rng.standard_normal(op.P), 0.0)
    d0 = np.where(dm, alpha * rng.standard_normal(op.D), 0.0)
    ccls = (balanced_classes(op.kids.size, rng) + rot) % 3
    lcls = (balanced_classes(op.leaves.size, rng) + rot) % 3
    for nodes, E, cls in ((op.kids, op.E6, ccls), (op.leaves, op.E13, lcls)):
        d0[E[nodes[cls == 0]]] = alpha * T
        d0[E[nodes[cls == 1]]] = -alpha * T
    return p0, d0, ccls, lcls


PRIMAL_SEGMENTS = ("x", "u", "y", "tau", "s")
DUAL_SEGMENTS = ("eta1", "eta2", "eta3", "eta4", "eta5", "eta6", "eta7", "eta11", "eta12", "eta13", "eta14")


def segment_rel_err(got, ref, op, kind=None):
    """{segment: max |got - ref| over the segment / the segment's own largest |ref| entry} of a
    flat primal (x, u, y, tau, s) or dual (eta1..eta7, eta11..eta14); kind "primal" or "dual",
    or None to tell them apart by length (refused where the two lengths coincide). A
    segment whose reference is all zero (placeholders only) is measured against 1e-300: exact
    zeros give 0, anything else fails any bound."""
    got = np.asarray(got, dtype=float).reshape(-1)
    ref = np.asarray(ref, dtype=float).reshape(-1)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if kind is None:
        assert op.P != op.D, "primal and dual have one length here: pass kind"
        kind = "primal" if ref.size == op.P else "dual"
    assert kind in ("primal", "dual") and ref.size == (op.P if kind == "primal" else op.D), (kind, ref.size, op.P, op.D)
    if kind == "primal":
        names, edges = PRIMAL_SEGMENTS, [op.X0, op.U0, op.Y0, op.T0, op.S0, op.P]
    else:
        names, edges = DUAL_SEGMENTS, [int(o[0]) for o in op.d_off] + [op.D]
    out = {}
    for k, name in enumerate(names):
        a, b = got[edges[k]:edges[k + 1]], ref[edges[k]:edges[k + 1]]
        out[name] = float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300)) if b.size else 0.0
    return out


def trace_rel_err(a, b):
    a = np.atleast_2d(a)
    b = np.atleast_2d(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)))
