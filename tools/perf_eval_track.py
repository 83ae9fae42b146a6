"""What the in-training greedy evaluation costs -> profiles/eval_track_perf.json.

    iteration  ms per train_iteration() (HIP events around each call) at
                   c2   256 envs x 64 steps, LSTM h = 64
                   c3   4096 envs x 128 steps, LSTM h = 128
               with the option off, and with --parent PATH (a built checkout of the parent commit) in that tree.  Every measurement
               is a FRESH process; the processes of a shape alternate parent, off | off, parent | ..., and a process reports the
               median of its rounds.  The yardstick is the range of the parent's own process medians.
    run        one EvalTracker.run() -- 1024 evaluation envs, the env's own step limit, an h = 128 LSTM and the MLP -- between two
               HIP events and on the host's clock up to the end of the device's work, against evaluate() (evaluate_with_lstm.py)
               of the parent tree (this tree without --parent) on the same policy and env arguments, on the host's clock (it reads
               the device as it goes).  The same process also runs tracker.run() under torch.cuda.set_sync_debug_mode("error") and
               says whether the installed torch raises on a deliberate .item() in that mode (i.e. whether the mode proves anything).
    kernels    us per call of the three entry points alone (uav_greedy_reduce on a 1024 x 250 x 6 chunk, uav_greedy_summary on 1024
               envs, uav_keep_best on the C3 LSTM policy's parameters, improving and not), each between two HIP events.
    every50    one tracker.run() at the trainer's defaults (256 evaluation envs, the env's step limit) on a C3 trainer, HIP events:
               divided by 50 it is what eval_every=50 adds to an iteration on average.
    launches   with --parent: one `rocprofv3 --kernel-trace --stats` run per tree of ten train_iteration() calls at C2 with the
               option off: the tables of kernel names and call counts must be equal.

    python tools/perf_eval_track.py [--parent PATH] [--what iteration,run,kernels,every50,launches] [--out profiles/eval_track_perf.json]
                                    [--rounds 20] [--warmup 5] [--repeats 3]
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
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"c2": dict(N=256, T=64, policy="lstm", H=64), "c3": dict(N=4096, T=128, policy="lstm", H=128)}
RUN_ENVS = 1024
TRACE_ITERS = 10
DEV = "cuda:0"


def _summary(xs, unit):
    xs = sorted(xs)
    return {"median_" + unit: statistics.median(xs), "min_" + unit: xs[0], "max_" + unit: xs[-1], "n": len(xs)}


def _paths(tree):
    sys.path[:0] = [tree, os.path.join(tree, "uav-wrf-les-ppo-lstm_amd")]


def _timed(torch, f):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    f()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def child_iteration(tree, shape, _state, warmup, rounds):
    _paths(tree)
    import torch
    from uavppo.trainer import VecPPOTrainer
    s = SHAPES[shape]
    tr = VecPPOTrainer(s["N"], s["T"], s["policy"], hidden=s["H"], device=DEV, seed=1)
    ms = [_timed(torch, tr.train_iteration) for _ in range(warmup + rounds)][warmup:]
    tr.losses()
    print(json.dumps(_summary(ms, "ms")), flush=True)


def child_trace(tree, shape, _state, _warmup, _rounds):
    _paths(tree)
    import torch
    from uavppo.trainer import VecPPOTrainer
    s = SHAPES[shape]
    tr = VecPPOTrainer(s["N"], s["T"], s["policy"], hidden=s["H"], device=DEV, seed=7)
    for _ in range(TRACE_ITERS):
        tr.train_iteration()
    torch.cuda.synchronize()
    tr.losses()


def child_evaluate(tree, _shape, kind, warmup, rounds):
    """evaluate() of `tree` on the policy a seed-1 trainer of that kind starts with, RUN_ENVS envs of seed 4321: host clock."""
    _paths(tree)
    import torch
    from evaluate_with_lstm import evaluate
    from uavppo.trainer import VecPPOTrainer
    from uavppo.vec_env import VecMethaneEnv
    tr = VecPPOTrainer(64, 16, kind, hidden=128, device=DEV, seed=1)
    env = VecMethaneEnv(RUN_ENVS, "v2.0", DEV, seed=4321)
    ms = []
    for r in range(warmup + rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m = evaluate(tr.policy, env)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    out = _summary(ms[warmup:], "ms")
    out.update(successes=int(m["success"].sum()), steps=int(m["steps"].sum()))
    print(json.dumps(out), flush=True)


def child_run(tree, _shape, kind, warmup, rounds):
    _paths(tree)
    import torch
    from uavppo.trainer import VecPPOTrainer
    tr = VecPPOTrainer(64, 16, kind, hidden=128, device=DEV, seed=1, eval_every=1, eval_envs=RUN_ENVS)
    t = tr.eval_tracker
    dev_ms, host_ms = [], []
    for r in range(warmup + rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dev_ms.append(_timed(torch, lambda: t.run(r)))
        host_ms.append((time.perf_counter() - t0) * 1e3)
        t.curve()
    rows = t.curve(wait=True)
    out = {"route": t.route, "limit": t.limit, "chunk": t.chunk, "device": _summary(dev_ms[warmup:], "ms"),
           "host_until_done": _summary(host_ms[warmup:], "ms"), "successes": int(rows[-1]["sums"][1]), "steps": int(rows[-1]["sums"][2])}
    # does run() wait for the device?  torch's sync debug mode raises on a synchronising call where the build honours it
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    ran, honoured = True, False
    try:
        try:
            t.run(10 ** 6)
        except RuntimeError as e:
            ran = str(e)[:300]
        try:
            torch.zeros(1, device=DEV).item()
        except RuntimeError:
            honoured = True
    finally:
        torch.cuda.set_sync_debug_mode("default")
    out["sync_debug_mode"] = {"run_completed_under_error_mode": ran, "mode_raises_on_a_deliberate_item": honoured}
    print(json.dumps(out), flush=True)


def child_kernels(tree, _shape, _state, warmup, rounds):
    _paths(tree)
    import torch
    from uavppo import ops
    from uavppo.trainer import VecPPOTrainer
    n, k, D = RUN_ENVS, 250, 6
    g = torch.Generator(device=DEV).manual_seed(1)
    recs = {"flags": (torch.rand(n, k, device=DEV, generator=g) < 0.004).to(torch.uint8), "obs": torch.rand(n, k, D, device=DEV, generator=g),
            "pos": torch.rand(n, k, 2, device=DEV, generator=g) * 500}
    z = lambda dt, *s: torch.zeros(*s, dtype=dt, device=DEV)
    ep = [z(torch.int32, n), z(torch.uint8, n), z(torch.float64, n, 2)]
    src, sums, state = torch.rand(n, 2, device=DEV, dtype=torch.float64) * 500, z(torch.float64, ops.EVAL_SUM_N), z(torch.float64, ops.BEST_N)
    P = VecPPOTrainer(64, 16, "lstm", hidden=128, device=DEV, seed=1).policy.flat
    best = torch.zeros_like(P)
    better = torch.tensor([64.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.0, 0.0], dtype=torch.float64, device=DEV)

    def improving():
        better[1] += 1.0
        ops.keep_best(state, better, 1, P, best)

    calls = {"uav_greedy_reduce": lambda: (ep[1].zero_(), ops.greedy_reduce(recs, 0, *ep)),
             "uav_greedy_summary": lambda: ops.greedy_summary(*ep, src, 300, 40.0, sums),
             "uav_keep_best_not_improving": lambda: ops.keep_best(state, sums * 0, 1, P, best),
             "uav_keep_best_improving": improving}
    us = {c: [] for c in calls}
    for r in range(warmup + rounds):
        for c, f in calls.items():
            us[c].append(_timed(torch, f) * 1e3)
    out = {c: _summary(v[warmup:], "us") for c, v in us.items()}
    out["note"] = ("uav_greedy_reduce includes the zeroing of ep_state (one more launch), uav_keep_best_* the small torch launch that "
                   "makes its row; uav_keep_best is two launches")
    out["parameters"], out["chunk"] = P.numel(), [n, k, D]
    print(json.dumps(out), flush=True)


def child_every50(tree, shape, _state, warmup, rounds):
    _paths(tree)
    import torch
    from uavppo.trainer import VecPPOTrainer
    s = SHAPES[shape]
    tr = VecPPOTrainer(s["N"], s["T"], s["policy"], hidden=s["H"], device=DEV, seed=1, eval_every=1)
    tr.eval["eval_every"] = 10 ** 9                       # the iterations themselves run without it
    it_ms, ev_ms = [], []
    for r in range(warmup + rounds):
        it_ms.append(_timed(torch, tr.train_iteration))
        ev_ms.append(_timed(torch, lambda: tr.eval_tracker.run(r)))
        tr.eval_tracker.curve()
    a, b = _summary(it_ms[warmup:], "ms"), _summary(ev_ms[warmup:], "ms")
    print(json.dumps({"train_iteration": a, "tracker_run": b, "eval_envs": tr.eval_tracker.N, "limit": tr.eval_tracker.limit,
                      "added_per_iteration_at_eval_every_50_ms": b["median_ms"] / 50.0,
                      "added_fraction_of_an_iteration": b["median_ms"] / 50.0 / a["median_ms"]}), flush=True)


CHILDREN = {"iteration": child_iteration, "trace": child_trace, "evaluate": child_evaluate, "run": child_run, "kernels": child_kernels,
            "every50": child_every50}


def run_child(mode, tree, shape, state, a, prefix=()):
    cmd = list(prefix) + [sys.executable, os.path.abspath(__file__), "--child", mode, tree, shape, state, "--warmup", str(a.warmup),
                          "--rounds", str(a.rounds)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if r.returncode != 0:                               # nothing more is started on the device after a failure
        raise SystemExit(f"{cmd}: exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}")
    return r.stdout


def last_json(text):
    return json.loads(text.strip().splitlines()[-1])


def launch_table(tree, a):
    """{kernel name: calls} of child_trace under rocprofv3 (a run of its own: kernel trace only, the program behind `--`)."""
    with tempfile.TemporaryDirectory() as d:
        run_child("trace", tree, "c2", "off", a, prefix=("rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "trace", "--"))
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if len(files) != 1:
            raise SystemExit(f"rocprofv3 left {len(files)} kernel_stats.csv files under {d}: {files}")
        with open(files[0]) as f:
            return {r["Name"]: int(r["Calls"]) for r in csv.DictReader(f)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", nargs=4, metavar=("MODE", "TREE", "SHAPE", "STATE"))
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--what", default="iteration,run,kernels,every50,launches")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_track_perf.json"))
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    if a.child:
        return CHILDREN[a.child[0]](a.child[1], a.child[2], a.child[3], a.warmup, a.rounds)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("perf_eval_track.py measures on the GPU: none is visible")
    what = a.what.split(",")
    parent = os.path.abspath(a.parent) if a.parent else None
    out = {}
    if os.path.exists(a.out):                           # the parts may be measured in separate runs: keep what is there
        with open(a.out) as f:
            out = json.load(f)
    out.update({"device": torch.cuda.get_device_name(0), "compute_units": torch.cuda.get_device_properties(0).multi_processor_count,
                "torch": torch.__version__, "hip": torch.version.hip, "rounds": a.rounds, "warmup_rounds": a.warmup, "ranks": 1,
                "multi_rank": "not measured", "parent_tree_measured": bool(parent)})

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")

    for shape in (SHAPES if "iteration" in what else []):
        runs = {k: [] for k in (["parent"] if parent else []) + ["off"]}
        for i in range(a.repeats):
            pair = ([("parent", parent)] if parent else []) + [("off", ROOT)]
            for name, tree in (pair if i % 2 == 0 else pair[::-1]):      # parent, off | off, parent | ...: neither is always first
                runs[name].append(last_json(run_child("iteration", tree, shape, "off", a)))
        med = {k: [r["median_ms"] for r in v] for k, v in runs.items()}
        res = {"what": "ms per train_iteration(), the option off; one fresh process per entry of `runs`", "shape": SHAPES[shape], "runs": runs,
               "median_of_process_medians_ms": {k: statistics.median(v) for k, v in med.items()}}
        if parent:
            res["parent_range_ms"] = [min(med["parent"]), max(med["parent"])]
            res["off_within_parent_range"] = min(med["parent"]) <= res["median_of_process_medians_ms"]["off"] <= max(med["parent"])
        out.setdefault("iteration", {})[shape] = res
        print(shape, {k: [round(x, 4) for x in v] for k, v in med.items()}, file=sys.stderr, flush=True)
        save()
    if "run" in what:
        out["run"] = {"what": f"one EvalTracker.run() of {RUN_ENVS} envs against evaluate() of the {'parent' if parent else 'same'} tree on the same "
                              "policy and env arguments; one process each", "policies": {}}
        for kind in ("lstm", "mlp"):
            res = {"tracker_run": last_json(run_child("run", ROOT, "c3", kind, a)), "evaluate": last_json(run_child("evaluate", parent or ROOT, "c3", kind, a))}
            res["same_successes_and_steps"] = all(res["tracker_run"][k] == res["evaluate"][k] for k in ("successes", "steps"))
            out["run"]["policies"][kind] = res
            print("run", kind, res["tracker_run"]["device"]["median_ms"], "ms against evaluate()", res["evaluate"]["median_ms"], "ms",
                  file=sys.stderr, flush=True)
        save()
    if "kernels" in what:
        out["kernels"] = {"what": "us per entry-point call alone, HIP events around one call, one process", "calls": last_json(run_child("kernels", ROOT, "c3", "off", a))}
        save()
    if "every50" in what:
        out["every50"] = last_json(run_child("every50", ROOT, "c3", "off", a))
        print("every50", out["every50"]["added_per_iteration_at_eval_every_50_ms"], "ms per iteration", file=sys.stderr, flush=True)
        save()
    ok = True
    if "launches" in what and parent:
        tables = {"parent": launch_table(parent, a), "off": launch_table(ROOT, a)}
        same = tables["parent"] == tables["off"]
        out["launches"] = {"shape": SHAPES["c2"], "iterations": TRACE_ITERS, "kernels": len(tables["off"]), "calls": sum(tables["off"].values()),
                           "off_equals_parent": same,
                           "off_vs_parent": {n: [tables["parent"].get(n, 0), tables["off"].get(n, 0)] for n in sorted(set(tables["parent"]) | set(tables["off"]))
                                             if tables["parent"].get(n, 0) != tables["off"].get(n, 0)}}
        print("launch tables", "equal" if same else "DIFFERENT", out["launches"]["off_vs_parent"], file=sys.stderr, flush=True)
        ok &= same
        save()
    print(json.dumps(out), flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
