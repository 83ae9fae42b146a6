"""What running observation normalisation (normalise_obs, uavppo/obs_norm.py) costs -> profiles/obs_norm_perf.json.  The protocol
of tools/perf_reward_norm.py:

    update     ms per update() (epochs = 5, one minibatch, after a collect(), between two HIP events -- as train_iteration()
               runs it) at
                   c3_lstm   4096 envs x 128 steps, LSTM h = 128
                   c3_mlp    4096 envs x 128 steps, the fused MLP
               in two states of this tree -- `off` (the keyword at its default) and `on` (normalise_obs=True) -- and, with
               --parent PATH (a built checkout of the parent commit), in that tree, which only has `off`.  Every measurement is a
               FRESH process, the processes of a shape alternate parent, off | off, parent | ... and then `on`, and a process
               reports the median of its rounds.  The yardstick is the range of the parent's process medians; `off` is judged
               against it: the tool exits 1 when `off` lies outside it (or when the launch tables differ).
    kernels    us per call of the four entry points an iteration uses, alone at the C3 shape (uav_obs_stats over 4096 x 128 x 6;
               uav_obs_norm_merge; uav_obs_fold and uav_obs_unfold_grad on the 512 x 6 first layer), each between two HIP events,
               the median over the rounds of one process; and the flat copy the fold is preceded by.
    launches   with --parent: one `rocprofv3 --kernel-trace --stats` run per tree of ten train_iteration() calls at C2 (256 x 64,
               h = 64) with the option off: the tables of kernel names and call counts must be equal; a third run with the option
               on lists what it adds.

    python tools/perf_obs_norm.py [--parent PATH] [--what update,kernels,launches] [--out profiles/obs_norm_perf.json]
                                  [--rounds 20] [--warmup 5] [--repeats 4]
"""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"c3_lstm": dict(N=4096, T=128, policy="lstm", H=128), "c3_mlp": dict(N=4096, T=128, policy="mlp", H=128)}
STATES = {"off": {}, "on": dict(normalise_obs=True)}
EPOCHS = 5
TRACE_SHAPE, TRACE_ITERS = (256, 64, 64), 10
DEV = "cuda:0"


def _summary(xs):
    xs = sorted(xs)
    return {"median": statistics.median(xs), "min": xs[0], "max": xs[-1], "n": len(xs)}


def child_update(tree, shape, state, warmup, rounds):
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
    out = {k + "_ms": v for k, v in _summary(ms).items() if k != "n"}
    out["n"] = len(ms)
    if state == "on":
        hs = tr.obs_norm.host_stats()
        assert hs["count"] == float((warmup + rounds) * s["N"] * s["T"]) and hs["skipped"] == 0.0, hs
        out["inv_sigma"] = [float(v) for v in hs["inv_sigma"]]
    print(json.dumps(out), flush=True)


def child_kernels(tree, shape, _state, warmup, rounds):
    sys.path[:0] = [tree, os.path.join(tree, "uav-wrf-les-ppo-lstm_amd")]
    import torch
    from uavppo import ops
    from uavppo.trainer import VecPPOTrainer
    s = SHAPES[shape]
    tr = VecPPOTrainer(s["N"], s["T"], s["policy"], hidden=s["H"], device=DEV, seed=1, use_curriculum=False, normalise_obs=True)
    tr.collect()
    on, grad = tr.obs_norm, tr.policy.grad
    n = on.rows * on.D
    dw, db = grad[on._ow:on._ow + n].view(on.rows, on.D), grad[on._ob:on._ob + on.rows]
    calls = {"uav_obs_stats": lambda: ops.obs_stats(tr.buf["obs"], on.stats),
             "uav_obs_norm_merge": lambda: ops.obs_norm_merge(on.state, on.stats, on.mask, on.eps, on.mu, on.inv_sigma),
             "uav_obs_unfold_grad": lambda: ops.obs_unfold_grad(dw, db, on.mu, on.inv_sigma),
             "uav_obs_fold": lambda: ops.obs_fold(on.w, on.b, on.mu, on.inv_sigma, on.w_eff, on.b_eff, tr.guard.ranges[0:1]),
             "flat_copy": lambda: on._flat.copy_(on.master)}
    us = {k: [] for k in calls}
    for r in range(warmup + rounds):
        for k, f in calls.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            if r >= warmup:
                us[k].append(a.elapsed_time(b) * 1e3)
    print(json.dumps({k: {kk + ("_us" if kk != "n" else ""): vv for kk, vv in _summary(v).items()} for k, v in us.items()}), flush=True)


def child_trace(tree, _shape, state, _warmup, _rounds):
    sys.path[:0] = [tree, os.path.join(tree, "uav-wrf-les-ppo-lstm_amd")]
    import torch
    from uavppo.trainer import VecPPOTrainer
    N, T, H = TRACE_SHAPE
    tr = VecPPOTrainer(N, T, policy="lstm", hidden=H, device=DEV, seed=7, **STATES[state])
    for _ in range(TRACE_ITERS):
        tr.train_iteration()
    torch.cuda.synchronize()
    tr.losses()


CHILDREN = {"update": child_update, "kernels": child_kernels, "trace": child_trace}


def run_child(mode, tree, shape, state, a, prefix=()):
    cmd = list(prefix) + [sys.executable, os.path.abspath(__file__), "--child", mode, tree, shape, state, "--warmup", str(a.warmup),
                          "--rounds", str(a.rounds)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        raise SystemExit(f"{cmd}: exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}")
    return r.stdout


def last_json(text):
    return json.loads(text.strip().splitlines()[-1])


def launch_table(tree, state, a):
    """{kernel name: calls} of child_trace under rocprofv3 (a run of its own: kernel trace only, the program behind `--`)."""
    with tempfile.TemporaryDirectory() as d:
        run_child("trace", tree, "c2", state, a, prefix=("rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "trace", "--"))
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if len(files) != 1:
            raise SystemExit(f"rocprofv3 left {len(files)} kernel_stats.csv files under {d}: {files}")
        with open(files[0]) as f:
            return {r["Name"]: int(r["Calls"]) for r in csv.DictReader(f)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", nargs=4, metavar=("MODE", "TREE", "SHAPE", "STATE"))
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--what", default="update,kernels,launches")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "obs_norm_perf.json"))
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=4)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    a = ap.parse_args()
    if a.child:
        return CHILDREN[a.child[0]](a.child[1], a.child[2], a.child[3], a.warmup, a.rounds)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("perf_obs_norm.py measures on the GPU: none is visible")
    what = a.what.split(",")
    parent = os.path.abspath(a.parent) if a.parent else None
    out = {"what": "ms per update() after a collect(), HIP events; one fresh process per entry of `runs`, parent / off alternating, then on",
           "device": torch.cuda.get_device_name(0), "compute_units": torch.cuda.get_device_properties(0).multi_processor_count,
           "torch": torch.__version__, "hip": torch.version.hip, "epochs": EPOCHS, "rounds": a.rounds, "warmup_rounds": a.warmup,
           "ranks": 1, "multi_rank": "not measured", "learning_speed": "not measured", "shapes": {}}

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")

    ok = True
    for shape in (a.shapes.split(",") if "update" in what else []):
        runs = {k: [] for k in (["parent"] if parent else []) + list(STATES)}
        for i in range(a.repeats):
            pair = [("parent", parent)] if parent else []
            pair.append(("off", ROOT))
            for name, tree in (pair if i % 2 == 0 else pair[::-1]):      # parent, off | off, parent | ...: neither is always first
                runs[name].append(last_json(run_child("update", tree, shape, "off", a)))
        for _ in range(a.repeats):
            runs["on"].append(last_json(run_child("update", ROOT, shape, "on", a)))
        med = {k: [r["median_ms"] for r in v] for k, v in runs.items()}
        res = {"shape": SHAPES[shape], "runs": runs, "median_of_process_medians_ms": {k: statistics.median(v) for k, v in med.items()}}
        base = "parent" if parent else "off"
        m = res["median_of_process_medians_ms"]
        res["baseline"] = base
        res["baseline_range_ms"] = [min(med[base]), max(med[base])]          # range of the repeated baseline processes
        res["minus_baseline_ms"] = {k: m[k] - m[base] for k in m if k != base}
        res["on_overhead_percent_of_baseline"] = 100.0 * (m["on"] - m[base]) / m[base]
        if parent:
            res["off_within_parent_range"] = min(med["parent"]) <= m["off"] <= max(med["parent"])
            ok &= res["off_within_parent_range"]      # the absolute figures of a shape are comparable only when it holds
        out["shapes"][shape] = res
        print(shape, {k: [round(x, 4) for x in v] for k, v in med.items()}, file=sys.stderr, flush=True)
        save()
    if "kernels" in what:
        out["kernels"] = {"what": "us per call alone at 4096 x 128 (LSTM h = 128: first layer 512 x 6), HIP events around one call, one process; "
                                  "uav_obs_stats is a 4-byte memset and one launch; flat_copy is the torch copy of the master into policy.flat in front of every fold",
                          "calls": last_json(run_child("kernels", ROOT, "c3_lstm", "on", a))}
        print("kernels", out["kernels"]["calls"], file=sys.stderr, flush=True)
        save()
    if "launches" in what and parent:
        tables = {"parent": launch_table(parent, "off", a), "off": launch_table(ROOT, "off", a), "on": launch_table(ROOT, "on", a)}
        same = tables["parent"] == tables["off"]
        diff = lambda x, y: {n: [x.get(n, 0), y.get(n, 0)] for n in sorted(set(x) | set(y)) if x.get(n, 0) != y.get(n, 0)}
        out["launches"] = {"shape": list(TRACE_SHAPE), "iterations": TRACE_ITERS, "kernels": len(tables["off"]), "calls": sum(tables["off"].values()),
                           "off_equals_parent": same, "off_vs_parent": diff(tables["parent"], tables["off"]),
                           "on_vs_off": diff(tables["off"], tables["on"])}
        print("launch tables", "equal" if same else "DIFFERENT", out["launches"]["off_vs_parent"], "on adds", out["launches"]["on_vs_off"],
              file=sys.stderr, flush=True)
        ok &= same
        save()
    print(json.dumps(out), flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
