"""The float64 reference of the evaluation tests: the nested-AVaR cost, the epigraph value,
the box violation and the dynamics residual of a flat primal, in plain NumPy over an
OracleProblem's fields (anc, chs, nch, SQ / iSQ, SR / iSR, SP / iSP, A / iA, B / iB, cond,
alpha_r, nl_lo / nl_hi / nl_active, l_lo / l_hi / l_active).

AVaR is the greedy sorted fill of the ambiguity set {alpha mu <= p, mu >= 0, 1'mu = 1}: the
mass goes to the largest outcomes first, each child taking at most p_k / alpha. The library
computes the same value by the Rockafellar-Uryasev minimum, a different algorithm.
"""
import numpy as np


def avar(Z, p, alpha):
    """max of mu'Z over {alpha mu <= p, mu >= 0, 1'mu = 1} (risks.py:28-35); alpha = 0: max Z."""
    Z = np.asarray(Z, dtype=np.float64).reshape(-1)
    p = np.asarray(p, dtype=np.float64).reshape(-1)
    if np.isnan(Z).any():
        return float("nan")
    if alpha <= 0.0:
        return float(Z.max())
    left, val = 1.0, 0.0
    for k in np.argsort(-Z, kind="stable"):
        mu = min(p[k] / alpha, left)
        val += mu * Z[k]
        left -= mu
        if left <= 0.0:
            break
    return float(val)


def nanmax0(v):
    """max(v, 0) over an array, a NaN entry winning (numpy's max propagates it)."""
    v = np.asarray(v, dtype=np.float64).reshape(-1)
    return float(np.max(np.maximum(v, 0.0), initial=0.0)) if not np.isnan(v).any() else float("nan")


def evaluate(orc, z, x0):
    """(cost, s_0, box violation, dynamics residual, node values [n]) of the flat primal z."""
    n, m, nx, nu = orc.n, orc.m, orc.nx, orc.nu
    z = np.asarray(z, dtype=np.float64).reshape(-1)
    X = z[orc.X0:orc.X0 + n * nx].reshape(n, nx)
    U = z[orc.U0:orc.U0 + m * nu].reshape(m, nu)
    ell = np.zeros(n)
    dyn = [np.abs(X[0] - np.asarray(x0, dtype=np.float64).reshape(-1))]
    for j in range(1, n):
        a = orc.anc[j]
        ell[j] = np.sum((orc.SQ[orc.iSQ[j]] @ X[a]) ** 2) + np.sum((orc.SR[orc.iSR[j]] @ U[a]) ** 2)
        dyn.append(np.abs(X[j] - orc.A[orc.iA[j]] @ X[a] - orc.B[orc.iB[j]] @ U[a]))
    V = np.zeros(n)
    for l in range(m, n):
        V[l] = np.sum((orc.SP[orc.iSP[l]] @ X[l]) ** 2)
    for i in range(m - 1, -1, -1):
        ch = slice(orc.chs[i], orc.chs[i] + orc.nch[i])
        V[i] = avar(ell[ch] + V[ch], orc.cond[ch], orc.alpha_r[i])
    box = [np.zeros(1)]
    for i in np.flatnonzero(orc.nl_active):
        w = np.concatenate([X[i], U[i]])
        box += [orc.nl_lo[i] - w, w - orc.nl_hi[i]]
    for k in np.flatnonzero(orc.l_active):
        box += [orc.l_lo[k] - X[m + k], X[m + k] - orc.l_hi[k]]
    return float(V[0]), float(z[orc.S0]), nanmax0(np.concatenate(box)), nanmax0(np.concatenate(dyn)), V
