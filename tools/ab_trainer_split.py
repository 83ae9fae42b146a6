"""Is VecPPOTrainer with its curriculum link and range guard split out (uavppo/curriculum_link.py, uavppo/range_guard.py,
uavppo/mirror_ring.py) the trainer of the parent commit?  Three answers -> profiles/trainer_split_ab.json:

    parity     the seeded configurations of CONFIGS, six train_iteration() calls each with the curriculum on, in this tree and in
               the parent: the final flat parameters, both Adam moments, loss_sums (SHA-256 of their bytes), radius, bonus,
               episodes_done and successes_done must be identical
    launches   one `rocprofv3 --kernel-trace --stats` run per tree of ten iterations of 256 x 64, h = 64: the tables of kernel
               names and call counts must be equal (written beside the JSON as trainer_split_launches_{parent,this}.csv)
    time       ms per train_iteration() (host clock around ROUND_ITERS iterations that end in a device synchronise) at C2
               (256 x 64, h = 64: where host time shows) and C3 (4096 x 128, h = 128), the trees alternating parent, this |
               this, parent | ..., a process reporting the median of its rounds after warm-up.  The yardstick is the range of
               the parent's process medians.

Every run is a FRESH process (a tree is a set of modules and a library: two cannot share one).

    python tools/ab_trainer_split.py --parent PATH [--what parity,launches,time] [--out profiles/trainer_split_ab.json] [--repeats 4]
"""
import argparse
import csv
import glob
import hashlib
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
ITERS = 6
CONFIGS = {          # name -> (num_envs, horizon, trainer keywords, attributes set after construction)
    "lstm_h64": (256, 64, dict(policy="lstm", hidden=64), {}),
    "lstm_h128_shuffle_envs": (256, 64, dict(policy="lstm", hidden=128, num_minibatches=4, shuffle_envs=True), {}),
    "lstm_h128_bptt16": (256, 64, dict(policy="lstm", hidden=128, bptt_len=16), {}),
    "mlp": (256, 64, dict(policy="mlp"), {}),
    "mlp_inline_v10_rows": (256, 64, dict(policy="mlp", update_form="inline_v10", minibatch_rows=1024), {}),
    "lstm_h256x2": (64, 16, dict(policy="lstm", hidden=256, layers=2), {}),
    "host_curriculum": (256, 64, dict(policy="lstm", hidden=64, device_curriculum=False), {}),
    "main_stream_curriculum": (256, 64, dict(policy="lstm", hidden=64), dict(side_stream_curriculum=False)),
}
SHAPES = {"c2": (256, 64, 64), "c3": (4096, 128, 128)}
ROUND_ITERS, ROUNDS, WARMUP_ROUNDS = 10, 20, 3
TRACE_ITERS = 10


def _trainer(tree, N, T, kw, attrs=None, radius=None):
    sys.path[:0] = [tree, os.path.join(tree, "uav-wrf-les-ppo-lstm_amd")]
    from uavppo.trainer import VecPPOTrainer
    tr = VecPPOTrainer(N, T, device=DEV, seed=7, **kw)
    for k, v in (attrs or {}).items():
        setattr(tr, k, v)
    if radius is not None:
        tr.radius = radius
        tr.reset()
        if not tr.device_curriculum:
            tr.curriculum.current_radius = radius
    return tr


def child_parity(tree, name):
    import torch
    N, T, kw, attrs = CONFIGS[name]
    tr = _trainer(tree, N, T, kw, attrs, radius=200.0)      # episodes end in every rollout: the window fills, radius / bonus move
    for _ in range(ITERS):
        tr.train_iteration()
    torch.cuda.synchronize()
    tr.losses()                                     # raises on NaN
    sha = lambda t: hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()
    bonus = tr.bonus
    out = {"flat": sha(tr.policy.flat), "exp_avg": sha(tr.exp_avg), "exp_avg_sq": sha(tr.exp_avg_sq), "loss_sums": sha(tr.loss_sums),
           "radius": float(tr.radius).hex(), "bonus": float(bonus).hex(), "bonus_type": type(bonus).__name__,
           "episodes_done": int(tr.episodes_done), "successes_done": int(tr.successes_done)}
    print(json.dumps(out), flush=True)


def child_time(tree, shape):
    import torch
    N, T, H = SHAPES[shape]
    tr = _trainer(tree, N, T, dict(policy="lstm", hidden=H))
    ms = []
    for r in range(WARMUP_ROUNDS + ROUNDS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(ROUND_ITERS):
            tr.train_iteration()
        torch.cuda.synchronize()
        if r >= WARMUP_ROUNDS:
            ms.append((time.perf_counter() - t0) / ROUND_ITERS * 1e3)
    tr.losses()
    ms.sort()
    print(json.dumps({"median_ms": statistics.median(ms), "min_ms": ms[0], "max_ms": ms[-1], "n": len(ms)}), flush=True)


def child_trace(tree, _):
    import torch
    N, T, H = SHAPES["c2"]
    tr = _trainer(tree, N, T, dict(policy="lstm", hidden=H))
    for _ in range(TRACE_ITERS):
        tr.train_iteration()
    torch.cuda.synchronize()
    tr.losses()


CHILDREN = {"parity": child_parity, "time": child_time, "trace": child_trace}


def run_child(tree, mode, arg, prefix=()):
    cmd = list(prefix) + [sys.executable, os.path.abspath(__file__), "--child", tree, mode, arg]
    print("...", os.path.basename(tree) or tree, mode, arg, file=sys.stderr, flush=True)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        raise SystemExit(f"{cmd}: exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}")
    return r.stdout


def launch_table(tree):
    """{kernel name: calls} of child_trace under rocprofv3 (a run of its own: kernel trace only, the program behind `--`)."""
    with tempfile.TemporaryDirectory() as d:
        run_child(tree, "trace", "c2", prefix=("rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "trace", "--"))
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if len(files) != 1:
            raise SystemExit(f"rocprofv3 left {len(files)} kernel_stats.csv files under {d}: {files}")
        with open(files[0]) as f:
            return {r["Name"]: int(r["Calls"]) for r in csv.DictReader(f)}


def write_table(path, table):
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["Name", "Calls"])
        for name in sorted(table):
            w.writerow([name, table[name]])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", nargs=3, metavar=("TREE", "MODE", "ARG"))
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--what", default="parity,launches,time")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trainer_split_ab.json"))
    ap.add_argument("--repeats", type=int, default=4, help="timing processes per tree and shape")
    a = ap.parse_args()
    if a.child:
        return CHILDREN[a.child[1]](a.child[0], a.child[2])
    if not a.parent:
        raise SystemExit("ab_trainer_split.py compares with the parent commit: give --parent PATH (a built checkout)")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("ab_trainer_split.py runs on the GPU: none is visible")
    trees = {"parent": os.path.abspath(a.parent), "this": ROOT}
    outdir = os.path.dirname(os.path.abspath(a.out))
    os.makedirs(outdir, exist_ok=True)
    out = {"what": "VecPPOTrainer with CurriculumLink / RangeGuard split out against the parent commit, one fresh process per run", "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "hip": torch.version.hip,
           "seed": 7, "iterations": ITERS}

    def save():
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")

    ok = True
    what = a.what.split(",")
    if "parity" in what:
        out["parity"] = {}
        for name in CONFIGS:
            got = {k: json.loads(run_child(t, "parity", name).strip().splitlines()[-1]) for k, t in trees.items()}
            same = got["parent"] == got["this"]
            out["parity"][name] = {"shape": list(CONFIGS[name][:2]), "keywords": {**CONFIGS[name][2], **CONFIGS[name][3]},
                                   "identical": same, "this": got["this"], "parent": None if same else got["parent"]}
            print("parity", name, "identical" if same else f"DIFFERENT {got}", file=sys.stderr, flush=True)
            ok &= same
            save()
        out["parity_all_identical"] = all(v["identical"] for v in out["parity"].values())
    if "launches" in what:
        tables = {k: launch_table(t) for k, t in trees.items()}
        for k, tab in tables.items():
            write_table(os.path.join(outdir, f"trainer_split_launches_{k}.csv"), tab)
        same = tables["parent"] == tables["this"]
        out["launches"] = {"shape": list(SHAPES["c2"]), "iterations": TRACE_ITERS, "kernels": len(tables["this"]),
                           "calls": sum(tables["this"].values()), "tables_equal": same,
                           "differences": {n: [tables["parent"].get(n, 0), tables["this"].get(n, 0)]
                                           for n in sorted(set(tables["parent"]) | set(tables["this"]))
                                           if tables["parent"].get(n, 0) != tables["this"].get(n, 0)}}
        print("launch tables", "equal" if same else f"DIFFERENT {out['launches']['differences']}", file=sys.stderr, flush=True)
        ok &= same
        save()
    if "time" in what:
        out["time"] = {"method": f"host clock around {ROUND_ITERS} train_iteration() calls ending in a device synchronise; {ROUNDS} rounds after "
                                 f"{WARMUP_ROUNDS} warm-up rounds per process, {a.repeats} fresh processes per tree, alternating", "shapes": {}}
        for shape in SHAPES:
            runs = {"parent": [], "this": []}
            for i in range(a.repeats):
                for k in (("parent", "this") if i % 2 == 0 else ("this", "parent")):        # neither tree is always first
                    runs[k].append(json.loads(run_child(trees[k], "time", shape).strip().splitlines()[-1]))
            med = {k: [r["median_ms"] for r in v] for k, v in runs.items()}
            res = {"shape": list(SHAPES[shape]), "runs": runs, "process_medians_ms": med,
                   "median_of_process_medians_ms": {k: statistics.median(v) for k, v in med.items()},
                   "parent_range_ms": [min(med["parent"]), max(med["parent"])]}
            res["this_within_or_below_parent_range"] = res["median_of_process_medians_ms"]["this"] <= max(med["parent"])
            out["time"]["shapes"][shape] = res
            print("time", shape, {k: [round(x, 4) for x in v] for k, v in med.items()}, file=sys.stderr, flush=True)
            ok &= res["this_within_or_below_parent_range"]
            save()
    print(json.dumps(out), flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
