"""What every kind of context launches: kernel_info of ops 0, 1, 2, 6, 9, 10, 11, 12, 13, 14, 15, 16,
one line per op, for a fixed list of contexts. Run it on two builds (RAOCP_HIP_LIB selects the
library) and diff the outputs before and after a change to kernel selection: the listing must
not move unless the change means it to.

The contexts: recipe_main; configs 1-5; config 2 in fp32; config 2 under each switch that takes
a kernel generation out (RAOCP_DR, RAOCP_DRC, RAOCP_CP6, RAOCP_CP6 + RAOCP_CP4, RAOCP_CP3,
RAOCP_DYN_SPLIT, RAOCP_DYN_FOLD, RAOCP_DYN_PER_STAGE); config 4 under RAOCP_CP5=0; and config 2
as two shards (the kernels tests/test_gpu_shard.py pins, fused and two-launch, and the defaults)
with each shard's owned ranges. The switches are read at create, so every context gets a fresh
child process with its environment.

    python tools/plan_dump.py > plan.txt
"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPS = (0, 1, 2, 6, 9, 10, 11, 12, 13, 14, 15, 16)
SWITCHES = ("RAOCP_DR", "RAOCP_DRC", "RAOCP_CP3", "RAOCP_CP4", "RAOCP_CP5", "RAOCP_CP6", "RAOCP_DYN_SPLIT",
            "RAOCP_DYN_FOLD", "RAOCP_DYN_PER_STAGE")
# the kernels tests/test_gpu_shard.py pins on both sides of its parity checks
SHARD_PIN = {"RAOCP_DR": "0", "RAOCP_CP4": "0", "RAOCP_CP5": "0", "RAOCP_CP6": "0"}

# (label, recipe: "main" or a config number, dtype, environment, shards)
CONTEXTS = [("main", "main", "float64", {}, 0)]
CONTEXTS += [(f"config{k}", k, "float64", {}, 0) for k in range(1, 6)]
CONTEXTS += [("config2 fp32", 2, "float32", {}, 0)]
CONTEXTS += [("config2 " + " ".join(f"{k}={v}" for k, v in env.items()), 2, "float64", env, 0) for env in (
    {"RAOCP_DR": "0"}, {"RAOCP_DRC": "0"}, {"RAOCP_CP6": "0"}, {"RAOCP_DYN_SPLIT": "0"}, {"RAOCP_DYN_FOLD": "0"},
    {"RAOCP_DYN_PER_STAGE": "1"}, {"RAOCP_CP6": "0", "RAOCP_CP4": "0"}, {"RAOCP_CP3": "0"})]
CONTEXTS += [("config4 RAOCP_CP5=0", 4, "float64", {"RAOCP_CP5": "0"}, 0)]
CONTEXTS += [("config2 shard {}/2 fused", 2, "float64", SHARD_PIN, 2),
             ("config2 shard {}/2 two", 2, "float64", dict(SHARD_PIN, RAOCP_CP3="0"), 2),
             ("config2 shard {}/2 default", 2, "float64", {}, 2)]


def dump(label, ctx):
    for op in OPS:
        print(f"{label} op{op}: {ctx.native.kernel_info(op)}")


def child(index):
    sys.path.insert(0, os.path.join(ROOT, "raocp-toolbox_amd"))
    import raocp.core as core
    from raocp.problems import build_problem, recipe_config, recipe_main
    label, recipe, dtype, _, shards = CONTEXTS[index]
    _, prob = build_problem(recipe_main() if recipe == "main" else recipe_config(recipe, seed=0))
    if not shards:
        dump(label, core.Cache(prob, dtype=dtype))
        return
    for rank in range(shards):
        ctx = core.Cache(prob, dtype=dtype)
        ctx.native.shard(rank, shards)
        dump(label.format(rank), ctx)
        lo, hi = ctx.native.shard_owned()
        print(f"{label.format(rank)} owned: {[int(v) for v in lo]} {[int(v) for v in hi]}")


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        child(int(sys.argv[2]))
        return 0
    for index, (label, _, _, env, _) in enumerate(CONTEXTS):
        e = {k: v for k, v in os.environ.items() if k not in SWITCHES}
        e.update(env)
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(index)], env=e, text=True,
                           capture_output=True, timeout=600)
        sys.stdout.write(p.stdout)
        sys.stdout.flush()
        if p.returncode != 0:
            sys.stderr.write(f"{label}: exit status {p.returncode}\n{p.stderr[-2000:]}\n")
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
