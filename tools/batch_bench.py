#!/usr/bin/env python3
"""Batched CP solves against the loop they replace, on main.py's problem.

Two legs, each at B in {1, 16, 256, 1024}, pinned alpha, tol = 0, K = 200 iterations per solve:
  batch       one cp_batch_run call of B instances
  sequential  B cp_run calls, one after another, on one context
A leg the library does not have is skipped (the sequential leg needs only cp_run, so the same
tool times the commit before the batch entry points). Timing: wall clock bracketed with
raocp_device_synchronize, one discarded warm-up run, the median of 5.
Prints one JSON object; --out FILE also writes it there.

    python tools/batch_bench.py [--legs batch,sequential] [--B 1,16,256,1024] [--out FILE]
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
    ap.add_argument("--legs", default="batch,sequential")
    ap.add_argument("--B", default="1,16,256,1024")
    ap.add_argument("--K", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dtype", choices=["float64", "float32"], default="float64")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.dtype == "float32":
        # the float batch kernel is opt-in; RAOCP_CPB=0 still selects the sequential fallback
        os.environ.setdefault("RAOCP_CPB_F32", "1")
    import raocp.core as core
    from raocp.core._native import device_synchronize
    from raocp.problems import build_problem, recipe_main

    r = recipe_main()
    tree, prob = build_problem(r)
    cache = core.Cache(prob, device=0, dtype=a.dtype)
    nat = cache.native
    alpha = 0.999 / nat.step_size()
    x0 = np.asarray(r["x0"], dtype=float).reshape(-1)
    K = a.K
    res = {"problem": "main.py (43 nodes, nx 3, nu 2)", "dtype": a.dtype, "K": K, "alpha": alpha, "reps": a.reps, "legs": {}}

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

    for leg in a.legs.split(","):
        if leg == "batch" and not hasattr(nat, "cp_batch_run"):
            res["legs"][leg] = "not available in this library"
            continue
        rows = {}
        for B in [int(v) for v in a.B.split(",")]:
            rng = np.random.default_rng(B)
            X = x0[None, :] * (0.1 + rng.random((B, 1)))
            if leg == "batch":
                fn = lambda: nat.cp_batch_run(X, K, 0.0, alpha)  # noqa: E731
            else:
                def fn():
                    for b in range(B):
                        nat.cp_run(X[b], K, 0.0, alpha)
            with contextlib.redirect_stdout(io.StringIO()):
                sec = timed(fn)
            rows[str(B)] = {"seconds": sec, "instance_iterations_per_s": B * (K + 1) / sec}
        res["legs"][leg] = rows
    if hasattr(nat, "cp_batch_run"):
        res["kernel"] = nat.kernel_info(13)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
