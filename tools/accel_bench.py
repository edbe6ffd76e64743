#!/usr/bin/env python3
"""Anderson-accelerated batch solves (k_cpa, accel = 5) against the plain batch kernel (k_cpb) on
main.py's problem.

Two measurements, each at B in {1, 256, 1024}:
  to_tolerance   cp_batch_run at tol = 1e-5, max_iters = 3000, the computed step: iterations to
                 the tolerance (min / median / max over the instances, and how many converged)
                 and the wall time of the call
  per_iteration  tol = 0, K = 200 iterations per solve: seconds per instance-iteration of either
                 kernel, and k_cpa's over k_cpb's
Instance 0 starts from x0 = (2, -1, -1); the others from that state scaled by 0.5 .. 1.
Timing: wall clock bracketed with raocp_device_synchronize, one discarded warm-up run, the median
of 5. Prints one JSON object; --out FILE also writes it there.

    python tools/accel_bench.py [--B 1,256,1024] [--out FILE]
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
    ap.add_argument("--B", default="1,256,1024")
    ap.add_argument("--K", type=int, default=200)
    ap.add_argument("--max-iters", type=int, default=3000)
    ap.add_argument("--tol", type=float, default=1e-5)
    ap.add_argument("--accel", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import raocp.core as core
    from raocp.core._native import device_synchronize
    from raocp.problems import build_problem, recipe_main

    tree, prob = build_problem(recipe_main())
    nat = core.Cache(prob, device=0).native
    alpha = 0.999 / nat.step_size()
    x0 = np.array([2.0, -1.0, -1.0])
    aa = (a.accel, 1, 1e-10, 1.0)
    res = {"problem": "main.py (43 nodes, nx 3, nu 2)", "alpha": alpha, "accel": a.accel, "reps": a.reps,
           "kernels": {"plain": nat.kernel_info(13), "accel": nat.kernel_info(19)}, "to_tolerance": {}, "per_iteration": {}}

    def timed(fn):
        out = fn()  # warm-up, discarded
        t = []
        for _ in range(a.reps):
            device_synchronize(0)
            t0 = time.perf_counter()
            out = fn()
            device_synchronize(0)
            t.append(time.perf_counter() - t0)
        return statistics.median(t), out

    for B in [int(v) for v in a.B.split(",")]:
        X = x0[None, :] * np.linspace(1.0, 0.5, B)[:, None]
        tt, pi = {}, {}
        for leg, opt in (("plain", None), ("accel", aa)):
            with contextlib.redirect_stdout(io.StringIO()):
                sec, (status, errs, _) = timed(lambda: nat.cp_batch_run(X, a.max_iters, a.tol, alpha, accel=opt))
                secK, _ = timed(lambda: nat.cp_batch_run(X, a.K, 0.0, alpha, accel=opt))
            it = np.array([e.shape[0] for e in errs])
            tt[leg] = {"seconds": sec, "converged": int(np.count_nonzero(status == 0)), "iterations_instance0": int(it[0]),
                       "iterations_min": int(it.min()), "iterations_median": float(np.median(it)), "iterations_max": int(it.max())}
            pi[leg] = {"seconds": secK, "seconds_per_instance_iteration": secK / (B * (a.K + 1))}
        pi["accel_over_plain"] = pi["accel"]["seconds"] / pi["plain"]["seconds"]
        tt["accel_over_plain_seconds"] = tt["accel"]["seconds"] / tt["plain"]["seconds"]
        res["to_tolerance"][str(B)] = tt
        res["per_iteration"][str(B)] = pi
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
