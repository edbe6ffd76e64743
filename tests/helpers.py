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


def crafted_start(op, alpha, seed, T=50.0, rot=0, calm=False):
    """(p0, d0) of a warm start whose first CP iteration takes every branch of the dual step:
    p0 standard normal on the live primal slots, d0 = alpha * standard normal on the live dual
    slots (zero on the placeholders, like every iterate the loop produces); every child cone
    and, by an independent shuffle, every leaf cone gets a class from a balanced seeded
    assignment: identity sets the cone's t entry (eta6 / eta13) of d0 to +alpha T, zero to
    -alpha T, scaling keeps the random value. rot rotates the classes (crafted_rotations).
    calm: a scaling cone's t entry of d0 is 0 instead, so that the t the iteration projects is the
    primal's half alone and stays clear of +-|F| on trees with hundreds of small cones, where some
    random t lands within the census margin of an edge for every seed.
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
        if calm:
            d0[E[nodes[cls == 2]]] = 0.0
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


def shard_ranges(op, S, R):
    """(own_lo, own_hi) per stage 0..N of each of R shards cut at stage S, on the host: what
    raocp_shard_owned returns after raocp_shard_setup (raocp_capi.hip:2401-2428: shard r's roots are
    stage S's ids [r nb / R, (r + 1) nb / R) in integer division, "owned id range per stage: the whole
    stage above the cut, descendants below")."""
    first = np.array([int(np.flatnonzero(op.stage == t)[0]) for t in range(op.N + 1)] + [op.n])
    nb = int(first[S + 1] - first[S])
    assert 1 <= S <= op.N and nb >= R >= 1, (S, nb, R)
    out = []
    for r in range(R):
        lo, hi = int(first[S] + r * nb // R), int(first[S] + (r + 1) * nb // R)
        own_lo, own_hi = list(first[:S]), list(first[1:S + 1])
        for t in range(S, op.N + 1):
            own_lo.append(lo)
            own_hi.append(hi)
            if t < op.N and hi > lo:
                lo, hi = int(op.chs[lo]), int(op.chs[hi - 1] + op.nch[hi - 1])
        out.append((np.array(own_lo, dtype=np.int64), np.array(own_hi, dtype=np.int64)))
    return out


def _node_entries(starts, sizes, nodes):
    """Flat indices of the blocks [starts[i], starts[i] + sizes[i]) of the given nodes."""
    starts, sizes = np.asarray(starts, np.int64)[nodes], np.asarray(sizes, np.int64)[nodes]
    if starts.size == 0:
        return np.zeros(0, np.int64)
    return np.repeat(starts - np.concatenate([[0], np.cumsum(sizes)[:-1]]), sizes) + np.arange(sizes.sum())


def shard_masks(op, own_lo, own_hi, S):
    """(primal mask, dual mask) of the entries of the flat primal and dual a shard answers for after
    a run, from its owned id range per stage (shard_owned) and its cut stage S.

    The rule restates raocp_shard_setup (raocp_capi.hip:2412-2428): a shard holds every node of the
    stages above the cut (own_lo / own_hi of a stage t < S are the whole stage) and, from the cut
    down, the descendants of its own roots. An entry goes with the node whose work item computes it:
      x, u, y, tau, s                  the node itself (u, y: nonleaf nodes);
      eta1, eta2, eta7                 the node as parent (its family's dual rows);
      eta3 .. eta6                     the node as child (its own cone);
      eta11 .. eta14                   the node as leaf;
    and only live slots count (OracleProblem.live_masks: the (1, 1) placeholders are nobody's).
    At the cut the kernels keep more than this in every shard: the cut's parents' families run
    replicated in the second CP launch (cp3_tb / cp5_tkb over [stage_ptr[S - 1], stage_ptr[S]),
    raocp_capi.hip:2460, 2478), which writes tau, s and eta3 .. eta6 of every root, and X1 scatters
    every root's eta2 (k_unpack_x1). Those copies are not claimed here: the owner's copy is the one
    its own subtree reads, so each such entry is held to account exactly once, in its owner, and
    below the top the masks of the shards are disjoint."""
    own_lo, own_hi = np.asarray(own_lo, np.int64), np.asarray(own_hi, np.int64)
    assert own_lo.size == own_hi.size == op.N + 1 and 1 <= S <= op.N
    node = np.zeros(op.n, dtype=bool)
    for a, b in zip(own_lo, own_hi):
        node[a:b] = True
    assert node[op.stage < S].all(), "the stages above the cut are replicated whole"
    return _masks_of_nodes(op, node)


def shard_top_masks(op, S):
    """(primal mask, dual mask) of the part of shard_masks every shard holds a copy of: the entries
    of the nodes of the stages above the cut, by the same rule."""
    return _masks_of_nodes(op, op.stage < S)


def _masks_of_nodes(op, sel):
    ids = np.flatnonzero(sel)
    par, kid, leaf = ids[ids < op.m], ids[ids >= 1], ids[ids >= op.m]
    pm, dm = np.zeros(op.P, dtype=bool), np.zeros(op.D, dtype=bool)
    for k, who in enumerate((ids, par, par, ids, ids)):
        starts = np.concatenate([[0], np.cumsum(op.p_sizes[k])[:-1]]) + (op.X0, op.U0, op.Y0, op.T0, op.S0)[k]
        pm[_node_entries(starts, op.p_sizes[k], who)] = True
    for k, who in enumerate((par, par, kid, kid, kid, kid, par, leaf, leaf, leaf, leaf)):
        dm[_node_entries(op.d_off[k], op.d_sizes[k], who)] = True
    live_p, live_d = op.live_masks()
    return pm & live_p, dm & live_d


def masked_segment_rel_err(got, ref, op, kind, mask):
    """segment_rel_err restricted to a mask: per segment, max |got - ref| over the segment's masked
    entries / the segment's own largest |ref| entry (over the whole segment, as segment_rel_err
    scales it, so the masked figure is held to the same bound)."""
    got = np.asarray(got, dtype=float).reshape(-1)
    ref = np.asarray(ref, dtype=float).reshape(-1)
    assert got.shape == ref.shape == mask.shape and kind in ("primal", "dual")
    if kind == "primal":
        names, edges = PRIMAL_SEGMENTS, [op.X0, op.U0, op.Y0, op.T0, op.S0, op.P]
    else:
        names, edges = DUAL_SEGMENTS, [int(o[0]) for o in op.d_off] + [op.D]
    out = {}
    for k, name in enumerate(names):
        sl = slice(edges[k], edges[k + 1])
        a, b, w = got[sl], ref[sl], mask[sl]
        out[name] = float(np.max(np.abs(a[w] - b[w])) / max(np.max(np.abs(b)), 1e-300)) if w.any() else 0.0
    return out


def trace_rel_err(a, b):
    a = np.atleast_2d(a)
    b = np.atleast_2d(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)))
