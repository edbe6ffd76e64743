"""NumPy model of the Anderson-accelerated batch solve (Solver.chock_batch(accel=m), k_cpa),
written over OracleProblem.cp_iteration. DESIGN.md section 4.7b states the algorithm.

v = (z, eta), T(v) one CP iteration, g_k = T(v_k), r_k = g_k - v_k. Two modes:

* free (log=None): the model solves for gamma and takes every decision itself;
* replay (log = Solver.batch_accel_log[b]): the trial decisions, the proposals and gamma come
  from the device's log, the model supplies T, the history and both sides of every inequality.

A log record is 12 doubles: [code, j, prop, |r_k|_2, gamma[8]] with code 0 plain, 1 proposal made,
2 trial accepted, 3 trial rejected, 4 solve refused; prop 0 none, 1 proposal made, 2 solve refused
in this iteration (an accepted trial keeps code 2 and says in prop what followed it); j the
column count when the solve ran (else the count after the push); gamma in column order, oldest
first, zero beyond j.
"""
import numpy as np

REC = 12


def aa_system(dR, r, reg):
    """(Gbar, b) of the columns dR (oldest first) and the residual r."""
    A = np.array(dR)
    G = A @ A.T
    b = A @ r
    j = len(dR)
    Gb = G.copy()
    Gb[np.diag_indices(j)] += reg * (np.trace(G) / j)   # the diagonal only: reg = inf leaves the rest finite
    return Gb, b


def aa_solve(Gb, b):
    """gamma = Gbar^-1 b by Cholesky, or None when a pivot is not positive or gamma not finite."""
    j = len(b)
    L = np.zeros((j, j))
    for c in range(j):
        d = Gb[c, c] - L[c, :c] @ L[c, :c]
        if not (d > 0.0) or not np.isfinite(d):
            return None
        L[c, c] = np.sqrt(d)
        for i in range(c + 1, j):
            L[i, c] = (Gb[i, c] - L[i, :c] @ L[c, :c]) / L[c, c]
    y = np.zeros(j)
    for i in range(j):
        y[i] = (b[i] - L[i, :i] @ y[:i]) / L[i, i]
    g = np.zeros(j)
    for i in range(j - 1, -1, -1):
        g[i] = (y[i] - L[i + 1:, i] @ g[i + 1:]) / L[i, i]
    return g if np.all(np.isfinite(g)) else None


class Result:
    pass


def run(orc, x0, alpha, max_iters, tol, m=5, every=1, reg=1e-10, safeguard=1.0, log=None, p0=None, d0=None):
    """The accelerated solve of one instance. Returns a Result with status, err / derr (one row per
    iteration), z / eta (the last T(.) computed), zprev / etaprev (the point it was computed
    from), log (records as above), trials [(k, lhs, rhs, code)], systems [(k, Gbar, b, gamma)]."""
    x0 = np.asarray(x0, dtype=float).reshape(-1)
    P = orc.P
    z = orc.initial_primal(x0) if p0 is None else np.array(p0, dtype=float)
    z[orc.X0:orc.X0 + orc.nx] = x0
    e = np.zeros(orc.D) if d0 is None else np.array(d0, dtype=float)
    v = np.concatenate([z, e])
    dG, dR, prev, pending = [], [], None, None
    out = Result()
    errs, derrs, recs, out.trials, out.systems = [], [], [], [], []
    k = 0
    while True:
        zp, ep, err, derr = orc.cp_iteration(v[:P], v[P:], alpha, x0)
        g = np.concatenate([zp, ep])
        r = g - v
        rn = float(np.sqrt(r @ r))
        errs.append(err)
        derrs.append(derr)
        rec = np.zeros(REC)
        rec[3] = rn
        vprev = v
        rejected = False
        if pending is not None:
            sg, srn = pending
            pending = None
            accept = rn <= safeguard * srn
            if log is not None:
                accept = int(log[k][0]) == 2
            out.trials.append((k, rn, safeguard * srn, 2 if accept else 3))
            rec[0] = 2 if accept else 3
            rejected = not accept
        stop = k >= max_iters or (not rejected and max(err) <= tol)
        if rejected and not stop:
            dG, dR, prev = [], [], None
            recs.append(rec)
            v = sg
            k += 1
            continue
        if not stop and not rejected:
            if prev is not None:
                dG.append(g - prev[0])
                dR.append(r - prev[1])
                dG, dR = dG[-m:], dR[-m:]
            prev = (g, r)
            rec[1] = len(dR)
            v = g
            if dR and (k + 1) % every == 0:
                Gb, b = aa_system(dR, r, reg)
                if log is None:
                    gam = aa_solve(Gb, b)
                else:
                    gam = np.array(log[k][4:4 + len(dR)]) if int(log[k][2]) == 1 else None
                if gam is None:
                    dG, dR, prev = [], [], None
                    rec[2] = 2
                    if rec[0] == 0:
                        rec[0] = 4
                else:
                    out.systems.append((k, Gb, b, gam))
                    v = g - np.array(dG).T @ gam
                    pending = (g, rn)
                    rec[2] = 1
                    rec[4:4 + len(gam)] = gam
                    if rec[0] == 0:
                        rec[0] = 1
        recs.append(rec)
        if stop:
            break
        k += 1
    out.status = 0 if k < max_iters else 1
    out.iters = k + 1
    out.err, out.derr, out.log = np.array(errs), np.array(derrs), np.array(recs)
    out.z, out.eta = g[:P], g[P:]
    out.zprev, out.etaprev = vprev[:P], vprev[P:]
    return out
