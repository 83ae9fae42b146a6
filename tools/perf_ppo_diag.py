"""What the update diagnostics cost -> profiles/ppo_diag_perf.json.

ms per update() (epochs = 5, one minibatch, after a collect(), between two HIP events -- as train_iteration() runs it) at

    c3_lstm   4096 envs x 128 steps, LSTM h = 128
    c3_mlp    4096 envs x 128 steps, the fused MLP

in three states of this tree -- `off` (both keywords at their defaults), `diag` (diagnostics=True), `kl`
(target_kl=1e30: the per-epoch all-reduce-and-read of the early stop, which then never stops) -- and, with --parent PATH (a
built checkout of the parent commit), in that tree, which only has `off`.  Every measurement is a FRESH process (a tree is a
set of modules and a library: two cannot share one), the processes of a shape alternate parent, off | off, parent | ... and
then diag, kl | ..., and a process reports the median of its rounds.  The run-to-run spread the README quotes is the range of
the parent's process medians; `off` is judged against it.

    python tools/perf_ppo_diag.py [--parent PATH] [--out profiles/ppo_diag_perf.json] [--rounds 20] [--warmup 5] [--repeats 4]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"c3_lstm": dict(N=4096, T=128, policy="lstm", H=128), "c3_mlp": dict(N=4096, T=128, policy="mlp", H=128)}
STATES = {"off": {}, "diag": dict(diagnostics=True), "kl": dict(target_kl=1e30)}
EPOCHS = 5
DEV = "cuda:0"


def child(tree, shape, state, warmup, rounds):
    sys.path[:0] = [tree, os.path.join(tree, "uav-wrf-les-ppo-lstm_amd")]
    import torch
    from uavppo.trainer import VecPPOTrainer
    s = SHAPES[shape]
    tr = VecPPOTrainer(s["N"], s["T"], s["policy"], hidden=s["H"], device=DEV, seed=1, use_curriculum=False, epochs=EPOCHS, **STATES[state])
    ms = []
    for r in range(warmup + rounds):
        tr.collect()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        tr.update()
        b.record()
        b.synchronize()
        if r >= warmup:
            ms.append(a.elapsed_time(b))
        tr.iteration += 1
    tr.losses()                                     # raises on NaN
    if state != "off":
        d = tr.diagnostics()
        assert d["epochs_run"] == EPOCHS and not d["stopped_early"]
    ms.sort()
    print(json.dumps({"median_ms": statistics.median(ms), "min_ms": ms[0], "max_ms": ms[-1], "n": len(ms)}), flush=True)


def run_child(tree, shape, state, a):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", tree, shape, state, "--warmup", str(a.warmup), "--rounds", str(a.rounds)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        raise SystemExit(f"{cmd}: exit {r.returncode}\n{r.stderr[-3000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", nargs=3, metavar=("TREE", "SHAPE", "STATE"))
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ppo_diag_perf.json"))
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=4)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    a = ap.parse_args()
    if a.child:
        return child(a.child[0], a.child[1], a.child[2], a.warmup, a.rounds)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("perf_ppo_diag.py measures on the GPU: none is visible")
    out = {"what": "ms per update() after a collect(), HIP events; one fresh process per entry of `runs`, parent / off and diag / kl alternating",
           "device": torch.cuda.get_device_name(0), "compute_units": torch.cuda.get_device_properties(0).multi_processor_count,
           "torch": torch.__version__, "hip": torch.version.hip, "epochs": EPOCHS, "rounds": a.rounds, "warmup_rounds": a.warmup, "shapes": {}}
    for shape in a.shapes.split(","):
        runs = {k: [] for k in (["parent"] if a.parent else []) + list(STATES)}
        for i in range(a.repeats):
            pair = [("parent", os.path.abspath(a.parent))] if a.parent else []
            pair.append(("off", ROOT))
            for name, tree in (pair if i % 2 == 0 else pair[::-1]):      # parent, off | off, parent | ...: neither is always first
                runs[name].append(run_child(tree, shape, "off", a))
        for _ in range(a.repeats):
            runs["diag"].append(run_child(ROOT, shape, "diag", a))
            runs["kl"].append(run_child(ROOT, shape, "kl", a))
        med = {k: [r["median_ms"] for r in v] for k, v in runs.items()}
        res = {"shape": SHAPES[shape], "runs": runs, "median_of_process_medians_ms": {k: statistics.median(v) for k, v in med.items()}}
        base = "parent" if a.parent else "off"
        res["baseline"] = base
        res["baseline_spread_ms"] = max(med[base]) - min(med[base])          # range of the repeated baseline processes
        m = res["median_of_process_medians_ms"]
        res["minus_baseline_ms"] = {k: m[k] - m[base] for k in m if k != base}
        out["shapes"][shape] = res
        print(shape, {k: [round(x, 4) for x in v] for k, v in med.items()}, "spread", round(res["baseline_spread_ms"], 4), file=sys.stderr, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
