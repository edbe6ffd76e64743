#!/usr/bin/env python3
"""Closed-loop MPC simulation of a batch against the host-driven loop it replaces, on main.py's
problem.

Two legs on the same library, each at B in {16, 256, 1024}, T = 20 steps, K = 50 iterations per
solve, pinned alpha, tol = 0, warm starts, the same seeded scenario paths:
  resident   one cp_batch_mpc call (k_cpb launches + one k_mpc_step launch per step)
  host_loop  the loop a caller writes without it: per step cp_batch_run with z0 / eta0, B calls
             of cp_batch_get, cp_batch_first_inputs and a NumPy plant step
Both legs are checked to produce the same states before they are timed. Timing: wall clock
bracketed with raocp_device_synchronize, one discarded warm-up run, the median of 5 (DESIGN.md
section 7). Prints one JSON object; --out FILE also writes it there.

    python tools/mpc_bench.py [--legs resident,host_loop] [--B 16,256,1024] [--out FILE]

--accel M (1 .. 8; off by default) measures something else with the same protocol (the same x0
distribution, seeded paths, pinned alpha, warm starts, one discarded run and the median of --reps
between raocp_device_synchronize calls): one cp_batch_mpc call per leg,
  plain      k_cpb + k_mpc_step, as `resident` above
  accel      k_cpa with memory M + k_mpc_step_aa (a trial every iteration, reg 1e-10, safeguard 1)
both at --tol (default 0: every solve runs K + 1 iterations). Per B and leg it reports the wall
time, the fraction of instances converged (status 0) at each step, the iterations of a solve
(min / median / max over all B x T solves and the median per step) and, for `accel`, the totals
of accel_counts (proposals, trials accepted, trials rejected, solves refused). --legs is ignored.

    python tools/mpc_bench.py --accel 5 [--tol 1e-5] [--K 50] [--B 256] [--out FILE]
"""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "raocp-toolbox_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="resident,host_loop")
    ap.add_argument("--B", default="16,256,1024")
    ap.add_argument("--T", type=int, default=20)
    ap.add_argument("--K", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dtype", choices=["float64", "float32"], default="float64")
    ap.add_argument("--out", default=None)
    ap.add_argument("--accel", type=int, default=0)
    ap.add_argument("--tol", type=float, default=0.0, help="with --accel only")
    a = ap.parse_args()
    if a.dtype == "float32":
        # the float kernels are opt-in; RAOCP_CPB=0 still selects the host loop over sequential solves
        os.environ.setdefault("RAOCP_CPB_F32", "1")
    import raocp.core as core
    from raocp.core._native import device_synchronize
    from raocp.core.solver import sample_scenarios
    from raocp.problems import build_problem, recipe_main

    r = recipe_main()
    tree, prob = build_problem(r)
    cache = core.Cache(prob, device=0, dtype=a.dtype)
    nat = cache.native
    alpha = 0.999 / nat.step_size()
    x0 = np.asarray(r["x0"], dtype=float).reshape(-1)
    K, T = a.K, a.T
    children = [int(i) for i in tree.children_of(0)]
    A = np.stack([np.asarray(prob.state_dynamics_at_node(i), dtype=float) for i in children])
    Bm = np.stack([np.asarray(prob.control_dynamics_at_node(i), dtype=float) for i in children])
    res = {"problem": "main.py (43 nodes, nx 3, nu 2)", "dtype": a.dtype, "T": T, "K": K, "alpha": alpha, "reps": a.reps, "legs": {}}

    def timed(fn):
        fn()  # warm-up, discarded
        t = []
        for _ in range(a.reps):
            device_synchronize(0)
            t0 = time.perf_counter()
            fn()
            device_synchronize(0)
            t.append(time.perf_counter() - t0)
        return statistics.median(t)

    def host_loop(X, scen):
        B = X.shape[0]
        x = X.copy()
        out = [x]
        z0 = e0 = None
        for t in range(T):
            nat.cp_batch_run(x, K, 0.0, alpha, z0, e0)
            u = nat.cp_batch_first_inputs()
            if t + 1 < T:
                pairs = [nat.cp_batch_get(b) for b in range(B)]
                z0 = np.array([p[0] for p in pairs])
                e0 = np.array([p[1] for p in pairs])
            j = scen[:, t]
            x = np.einsum("brk,bk->br", A[j], x) + np.einsum("brk,bk->br", Bm[j], u)
            out.append(x)
        return np.stack(out, axis=1)

    def solves(out):
        """What a run's solves did: out = cp_batch_mpc's tuple."""
        status, iters = out[3], out[4]
        d = {"converged_fraction_per_step": [float(v) for v in np.mean(status == 0, axis=0)],
             "iterations": {"min": int(iters.min()), "median": float(np.median(iters)), "max": int(iters.max())},
             "iterations_median_per_step": [float(v) for v in np.median(iters, axis=0)]}
        if len(out) > 6:
            d["accel_counts_total"] = dict(zip(("proposals", "accepted", "rejected", "refused"),
                                               (int(v) for v in out[6].sum(axis=(0, 1)))))
        return d

    if a.accel:
        aa = (a.accel, 1, 1e-10, 1.0)
        res["accel"] = {"m": a.accel, "every": 1, "reg": 1e-10, "safeguard": 1.0, "tol": a.tol}
        res["legs"] = {"plain": {}, "accel": {}}
        for B in [int(v) for v in a.B.split(",")]:
            rng = np.random.default_rng(B)
            X = x0[None, :] * (0.1 + rng.random((B, 1)))
            scen = sample_scenarios(tree.conditional_probabilities_of_children(0), B, T, seed=B)
            fns = {"plain": lambda: nat.cp_batch_mpc(X, scen, K, a.tol, alpha, True),             # noqa: E731
                   "accel": lambda: nat.cp_batch_mpc(X, scen, K, a.tol, alpha, True, accel=aa)}   # noqa: E731
            for leg, fn in fns.items():
                sec = timed(fn)
                d = {"seconds": sec, "ms_per_step": 1e3 * sec / T}
                d.update(solves(fn()))
                res["legs"][leg][str(B)] = d
        res["kernels"] = [nat.kernel_info(op) for op in (13, 14, 19, 20)]
        line = json.dumps(res)
        print(line)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(json.dumps(res, indent=1) + "\n")
        return

    legs = a.legs.split(",")
    for leg in legs:
        res["legs"][leg] = {}
    for B in [int(v) for v in a.B.split(",")]:
        rng = np.random.default_rng(B)
        X = x0[None, :] * (0.1 + rng.random((B, 1)))
        scen = sample_scenarios(tree.conditional_probabilities_of_children(0), B, T, seed=B)
        fns = {"resident": lambda: nat.cp_batch_mpc(X, scen, K, 0.0, alpha, True)[0],   # noqa: E731
               "host_loop": lambda: host_loop(X, scen)}                                  # noqa: E731
        with contextlib.redirect_stdout(io.StringIO()):
            if len(legs) == 2:
                xa, xb = fns[legs[0]](), fns[legs[1]]()
                scale = max(float(np.max(np.abs(xb))), 1e-300)
                res.setdefault("max_state_difference_rel", {})[str(B)] = float(np.max(np.abs(xa - xb))) / scale
            for leg in legs:
                sec = timed(fns[leg])
                res["legs"][leg][str(B)] = {"seconds": sec, "ms_per_step": 1e3 * sec / T,
                                            "instance_iterations_per_s": B * T * (K + 1) / sec}
    res["kernels"] = [nat.kernel_info(13), nat.kernel_info(14)]
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
