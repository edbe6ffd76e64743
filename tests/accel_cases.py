"""The option grid, the trees and the coverage conditions shared by tests/test_accel_host.py (CPU:
the free model of tests/accel_ref.py alone meets every condition) and tests/test_gpu_accel_grid.py
(GPU: k_cpa's log meets them, and the replay of that log agrees with the device).

A case is (tree, option set). The option sets, (m, every, reg, safeguard):

    m1       1  1  1e-10  1      the degenerate ring, (head + 1) % 1
    m2       2  1  1e-10  1
    m8       8  1  1e-10  1      every gamma slot and all 2 * 8 + 1 partial sums live
    m3e3     3  3  1e-10  1      columns pushed on iterations that do not solve
    m5e2r0   5  2  0      1      no regularisation
    m4r1e-2  4  1  1e-2   1      a large one
    m5s.5    5  1  1e-10  0.5    rejections and proposals mixed

The trees (tests/branch_cases.problem): main, s5x3 and m7x32 run the whole grid, the others m1, m8
and m3e3. Every solve is K = 40 iterations with tol = 0 from B = 3 initial states x0, 0.5 x0 and
-0.3 x0 (m7x32-dense: 0.75 x0 for the second, see SCALES_OF).
"""
import numpy as np

import branch_cases as bc

K = 40
SCALES = (1.0, 0.5, -0.3)
# m7x32-dense from 0.5 x0 with m = 8: the free model rejects the trials of iterations 15 and 28, so
# no 9 columns in a row are committed once the ring is full; from 0.75 x0 it rejects none
SCALES_OF = {"m7x32-dense": (1.0, 0.75, -0.3)}
OPTS = {"m1": (1, 1, 1e-10, 1.0), "m2": (2, 1, 1e-10, 1.0), "m8": (8, 1, 1e-10, 1.0), "m3e3": (3, 3, 1e-10, 1.0),
        "m5e2r0": (5, 2, 0.0, 1.0), "m4r1e-2": (4, 1, 1e-2, 1.0), "m5s.5": (5, 1, 1e-10, 0.5)}
FULL_TREES = ("main", "s5x3", "m7x32")
SOME_TREES = ("s1x1", "s17x5", "s16x16", "m7x32-dense", "g53")
SOME_OPTS = ("m1", "m8", "m3e3")
TREES = FULL_TREES + SOME_TREES
CASES = [(t, o) for t in FULL_TREES for o in OPTS] + [(t, o) for t in SOME_TREES for o in SOME_OPTS]
assert set(TREES) == set(bc.CPA_KERNEL)


def states(tree):
    """(3, nx): the tree's x0 times its scales."""
    x0 = np.asarray(bc.problem(tree)[0]["x0"], dtype=float).reshape(-1)
    return np.stack([s * x0 for s in SCALES_OF.get(tree, SCALES)])


def coverage_violations(log, opt):
    """The conditions a case's log ((rows, 12), of the device or of the free model) must meet for
    the case to exercise what it is for; returns the list of those it misses. Over the records
    before the one that stops the solve, with `cleared` a rejected trial or a refused solve and a
    `push` a record that is no rejection and has j >= 1 (a column is committed in exactly those):
      - j follows the ring: 0 at the start, after a clear and in a rejection, else min(j + 1, m);
      - some record has j == m and is followed by m + 1 pushes with no clear from that record on,
        one of them a proposal: every ring slot is overwritten and a solve reads the columns
        oldest first after the wrap (all sets but m5s.5: with a proposal every iteration such a
        run is some 2 m trials accepted in a row, each halving |r|_2 under its safeguard of 0.5,
        which no problem here does; that set is there for the next condition, and its ring is
        that of m = 5, which the suite's other tests and m5e2r0 fill);
      - every > 1: no record with (k + 1) % every != 0 proposes or refuses, and some of them
        commit a column while j < m;
      - m5s.5: at least 5 rejections and at least 5 proposals.
    The last record holds no column count, no proposal and no gamma."""
    m, every, reg, safeguard = OPTS[opt]
    log = np.atleast_2d(log)
    code, j, prop = (log[:, q].astype(int) for q in range(3))
    n = log.shape[0] - 1
    bad = []
    if j[n] != 0 or prop[n] != 0 or code[n] in (1, 4) or np.any(log[n, 4:] != 0):
        bad.append(f"the stopping record {log[n, :4].tolist()}")
    cleared = (code == 3) | (prop == 2)
    push = (code != 3) & (j >= 1)
    for k in range(n):
        want = 0 if (k == 0 or cleared[k - 1] or code[k] == 3) else min(j[k - 1] + 1, m)
        if j[k] != want:
            bad.append(f"record {k}: j = {j[k]}, the ring says {want}")
    full = [k for k in range(n) if j[k] == m and k + m + 1 < n and not cleared[k:k + m + 2].any()
            and push[k + 1:k + m + 2].all() and (prop[k + 1:k + m + 2] == 1).any()]
    if not full and opt != "m5s.5":
        bad.append(f"no record with j == {m} followed by {m + 1} pushes and a proposal without a clear")
    if every > 1:
        off = [k for k in range(n) if (k + 1) % every != 0]
        if any(prop[k] != 0 or code[k] in (1, 4) for k in off):
            bad.append(f"a proposal or a refusal off the cadence of {every}")
        if not any(push[k] and k > 0 and j[k] == j[k - 1] + 1 for k in off):
            bad.append("no column committed on an iteration that does not solve")
    if opt == "m5s.5":
        rej, props = int(np.count_nonzero(code[:n] == 3)), int(np.count_nonzero(prop[:n] == 1))
        if rej < 5 or props < 5:
            bad.append(f"{rej} rejections and {props} proposals, 5 of each wanted")
    return bad


def gamma_violations(log):
    """gamma is zero beyond j in every record and wholly zero where no proposal was made."""
    log = np.atleast_2d(log)
    bad = []
    for k, rec in enumerate(log):
        live = int(rec[1]) if int(rec[2]) == 1 else 0
        if np.any(rec[4 + live:] != 0.0):
            bad.append(f"record {k}: {rec.tolist()}")
    return bad


def refusals_of(rows, every):
    """Solves refused in a solve of `rows` iterations when every solve is refused: after a clear
    (and at the start) one iteration holds the pair, the next commits the first column, and the
    first iteration k >= 1 from there with (k + 1) % every == 0 solves and clears. every = 1: the
    odd k below the stopping record, (rows - 1) // 2 of them; every >= 2: every k = every - 1
    (mod every) below it, (rows - 1) // every of them."""
    return (rows - 1) // 2 if every == 1 else (rows - 1) // every
