"""What the KL-adaptive step size costs -> profiles/lr_control_perf.json.

    update     ms per update() (epochs = 5, one minibatch, after a collect(), between two HIP events -- as train_iteration()
               runs it) at
                   c3_lstm   4096 envs x 128 steps, LSTM h = 128
                   c3_mlp    4096 envs x 128 steps, the fused MLP
               in three states of this tree -- `off` (the keywords at their defaults), `diag` (diagnostics=True) and `adaptive`
               (lr_schedule="adaptive", which implies the diagnostics) -- and, with --parent PATH (a built checkout of the parent
               commit), in that tree, which only has `off`.  Every measurement is a FRESH process (a tree is a set of modules and
               a library: two cannot share one); the processes of a shape alternate parent, off | off, parent | ... and then
               diag, adaptive | adaptive, diag | ..., and a process reports the median of its rounds.  The yardstick is the range
               of the parent's process medians: `off` is judged against it, and `adaptive` minus `diag` against its width plus
               one uav_lr_adapt call.
    kernels    us per call of the three new entry points alone (uav_clip_adam_dlr on the C3 LSTM policy's parameters, with
               uav_clip_adam beside it: two launches each; uav_lr_adapt; uav_lr_init), each between two HIP events, the median
               over the rounds of one process.
    launches   with --parent: one `rocprofv3 --kernel-trace --stats` run per tree of ten train_iteration() calls at C2 (256 x 64,
               h = 64) with the keywords off: the tables of kernel names and call counts must be equal; two more runs list what
               `adaptive` launches that `diag` does not.

    python tools/perf_lr_control.py [--parent PATH] [--what update,kernels,launches] [--out profiles/lr_control_perf.json]
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
STATES = {"off": {}, "diag": dict(diagnostics=True), "adaptive": dict(lr_schedule="adaptive", desired_kl=0.01)}
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
    if state == "adaptive":
        st = tr.lr_control.state.cpu().tolist()
        assert sum(st[2:]) == float(warmup + rounds), st           # one decision per update
        out["lr_state"] = st
    print(json.dumps(out), flush=True)


def child_kernels(tree, shape, _state, warmup, rounds):
    sys.path[:0] = [tree, os.path.join(tree, "uav-wrf-les-ppo-lstm_amd")]
    import torch
    from uavppo import ops
    from uavppo.trainer import VecPPOTrainer
    s = SHAPES[shape]
    tr = VecPPOTrainer(s["N"], s["T"], s["policy"], hidden=s["H"], device=DEV, seed=1, use_curriculum=False, lr_schedule="adaptive", desired_kl=0.01)
    tr.train_iteration()
    c, row, grad = tr.lr_control, tr._diag_epochs[tr._diag_epochs_run - 1], tr.policy.grad
    p, m, v = tr.policy.flat.clone(), tr.exp_avg.clone(), tr.exp_avg_sq.clone()
    calls = {"uav_clip_adam": lambda: ops.clip_adam(p, grad, m, v, 1, 3e-5, gnorm_out=tr.gnorm),
             "uav_clip_adam_dlr": lambda: ops.clip_adam_dlr(p, grad, m, v, 1, c.lr_dev, gnorm_out=tr.gnorm),
             "uav_lr_adapt": lambda: c.adapt(row),
             "uav_lr_init": lambda: c.reset(3e-5)}
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
    out = {k: {kk + ("_us" if kk != "n" else ""): vv for kk, vv in _summary(v).items()} for k, v in us.items()}
    out["parameters"] = p.numel()
    print(json.dumps(out), flush=True)


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lr_control_perf.json"))
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=4)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    a = ap.parse_args()
    if a.child:
        return CHILDREN[a.child[0]](a.child[1], a.child[2], a.child[3], a.warmup, a.rounds)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("perf_lr_control.py measures on the GPU: none is visible")
    what = a.what.split(",")
    parent = os.path.abspath(a.parent) if a.parent else None
    out = {}
    if os.path.exists(a.out):                       # the parts may be measured in separate runs: keep what is there
        with open(a.out) as f:
            out = json.load(f)
    out.update({"what": "ms per update() after a collect(), HIP events; one fresh process per entry of `runs`, parent / off and diag / adaptive alternating",
                "device": torch.cuda.get_device_name(0), "compute_units": torch.cuda.get_device_properties(0).multi_processor_count,
                "torch": torch.__version__, "hip": torch.version.hip, "epochs": EPOCHS, "rounds": a.rounds, "warmup_rounds": a.warmup,
                "ranks": 1, "multi_rank": "not measured"})
    out.setdefault("shapes", {})

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")

    for shape in (a.shapes.split(",") if "update" in what else []):
        runs = {k: [] for k in (["parent"] if parent else []) + list(STATES)}
        for i in range(a.repeats):
            pair = [("parent", parent)] if parent else []
            pair.append(("off", ROOT))
            for name, tree in (pair if i % 2 == 0 else pair[::-1]):      # parent, off | off, parent | ...: neither is always first
                runs[name].append(last_json(run_child("update", tree, shape, "off", a)))
        for i in range(a.repeats):
            for name in (("diag", "adaptive") if i % 2 == 0 else ("adaptive", "diag")):
                runs[name].append(last_json(run_child("update", ROOT, shape, name, a)))
        med = {k: [r["median_ms"] for r in v] for k, v in runs.items()}
        res = {"shape": SHAPES[shape], "runs": runs, "median_of_process_medians_ms": {k: statistics.median(v) for k, v in med.items()}}
        base = "parent" if parent else "off"
        m = res["median_of_process_medians_ms"]
        res["baseline"] = base
        res["baseline_range_ms"] = [min(med[base]), max(med[base])]          # range of the repeated baseline processes
        res["minus_baseline_ms"] = {k: m[k] - m[base] for k in m if k != base}
        res["adaptive_minus_diag_ms"] = m["adaptive"] - m["diag"]
        res["diag_range_ms"] = [min(med["diag"]), max(med["diag"])]
        if parent:
            res["off_within_parent_range"] = min(med["parent"]) <= m["off"] <= max(med["parent"])
        out["shapes"][shape] = res
        print(shape, {k: [round(x, 4) for x in v] for k, v in med.items()}, file=sys.stderr, flush=True)
        save()
    if "kernels" in what:
        out["kernels"] = {"what": "us per entry-point call alone, HIP events around one call, one process (the two Adam forms are two launches each, "
                                  "on the C3 LSTM policy's parameters)",
                          "calls": last_json(run_child("kernels", ROOT, "c3_lstm", "adaptive", a))}
        print("kernels", out["kernels"]["calls"], file=sys.stderr, flush=True)
        save()
    ok = True
    if "launches" in what and parent:
        tables = {"parent": launch_table(parent, "off", a), "off": launch_table(ROOT, "off", a), "diag": launch_table(ROOT, "diag", a),
                  "adaptive": launch_table(ROOT, "adaptive", a)}
        same = tables["parent"] == tables["off"]
        diff = lambda x, y: {n: [x.get(n, 0), y.get(n, 0)] for n in sorted(set(x) | set(y)) if x.get(n, 0) != y.get(n, 0)}
        out["launches"] = {"shape": list(TRACE_SHAPE), "iterations": TRACE_ITERS, "kernels": len(tables["off"]), "calls": sum(tables["off"].values()),
                           "off_equals_parent": same, "off_vs_parent": diff(tables["parent"], tables["off"]),
                           "adaptive_vs_diag": diff(tables["diag"], tables["adaptive"])}
        print("launch tables", "equal" if same else "DIFFERENT", out["launches"]["off_vs_parent"], "adaptive against diag",
              out["launches"]["adaptive_vs_diag"], file=sys.stderr, flush=True)
        ok &= same
        save()
    print(json.dumps(out), flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
