#!/usr/bin/env python3
"""What one evaluation of a solve costs, next to one application of L on the same context.

Builds BASELINE config 2, 4 or 5, runs 10 CP iterations from x0 so that the context holds an
iterate of a solve, then times
  evaluate  the launches of one raocp_evaluate (k_eval_nodes and the sweep's launches) between two
            HIP events on the context's stream: raocp_op_bench(17, 1), the median of 20 after 3
            warm-ups
  ell       raocp_op_bench(0): L on device-resident vectors, 200 launches replayed as one graph
and prints one JSON line (--out FILE also writes it there). evaluate is timed launch by launch,
as a caller pays for it; L's figure is kernels back to back.

    python tools/eval_bench.py [--config 2|4|5] [--dtype float64|float32] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "raocp-toolbox_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, choices=[2, 4, 5], default=2)
    ap.add_argument("--dtype", choices=["float64", "float32"], default="float64")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import raocp.core as core
    from raocp.problems import build_problem, recipe_config

    r = recipe_config(a.config)
    tree, prob = build_problem(r)
    cache = core.Cache(prob, device=0, dtype=a.dtype)
    nat = cache.native
    x0 = np.asarray(r["x0"], dtype=float).reshape(-1)
    alpha = 0.999 / nat.step_size()
    nat.cp_run(x0, 9, 0.0, alpha)
    out = nat.evaluate()
    for _ in range(3):
        nat.op_bench(17, 1)
    t_eval = [nat.op_bench(17, 1) for _ in range(20)]
    t_ell = nat.op_bench(0, 200)
    pk = cache.packed
    res = {"tool": "eval_bench", "config": a.config, "dtype": a.dtype, "nodes": int(pk.n), "nx": int(pk.nx), "nu": int(pk.nu),
           "kernels": nat.kernel_info(17), "ell_kernel": nat.kernel_info(0),
           "evaluate_us": round(1e3 * statistics.median(t_eval), 2), "evaluate_us_min": round(1e3 * min(t_eval), 2),
           "evaluate_us_max": round(1e3 * max(t_eval), 2), "ell_us": round(1e3 * t_ell, 2),
           "ratio": round(statistics.median(t_eval) / t_ell, 2),
           "cost": float(out[0]), "s0": float(out[1]), "box_violation": float(out[2]), "dynamics_residual": float(out[3])}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
