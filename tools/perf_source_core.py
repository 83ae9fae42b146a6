"""The source-estimate kernels of this tree against a built checkout of the parent commit -> profiles/source_core_perf.json.

tools/perf_source_fit.py and tools/perf_source_stop.py time their `kernels` and `run` steps on their own tree only (--parent serves
their `iteration` and `launches` steps).  This driver starts those tools' own children (--child MODE TREE ...) in fresh processes
that alternate between the two trees in swapped order, --repeats times each, and compares per figure the median of this tree's
process medians with the spread (min .. max) of the parent's own process medians: that spread is the yardstick, as in
tools/ab_trainer_split.py.  tools/perf_source_aniso.py has neither --parent nor children: each tree's own copy of it runs whole
(kernels and run), alternating likewise.  --merge NAME=FILE puts the JSON another tool wrote (launch tables, resources) beside it.

    python tools/perf_source_core.py --parent PATH [--repeats 3] [--rounds 20] [--warmup 5] [--merge NAME=FILE ...]
                                     [--out profiles/source_core_perf.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, TOOLS)
import perf_eval_track as pet  # noqa: E402

# (name, tool, child mode, state)
STEPS = (("fit_kernels", "perf_source_fit.py", "kernels", "off"), ("fit_run", "perf_source_fit.py", "run", "on"),
         ("stop_kernels", "perf_source_stop.py", "kernels", "off"), ("stop_run", "perf_source_stop.py", "run", "source_stop"),
         ("stop_run_cannot_fire", "perf_source_stop.py", "run", "source_stop_cannot_fire"),
         ("aniso", "perf_source_aniso.py", None, None))


def child(tool, mode, tree, state, a):
    """one fresh process on `tree`: this tree's tool as a child of that mode, or (mode None) the tree's own copy of the tool, whole"""
    with tempfile.TemporaryDirectory() as d:
        res = os.path.join(d, "out.json")
        cmd = ([sys.executable, os.path.join(TOOLS, tool), "--child", mode, tree, "c3", state] if mode else
               [sys.executable, os.path.join(tree, "tools", tool), "--what", "kernels,run", "--out", res])
        r = subprocess.run(cmd + ["--warmup", str(a.warmup), "--rounds", str(a.rounds)], capture_output=True, text=True, timeout=300)
        if r.returncode != 0:                           # nothing more is started on the device after a failure
            raise SystemExit(f"{cmd}: exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}")
        if mode:
            return pet.last_json(r.stdout)
        with open(res) as f:
            return {k: v for k, v in json.load(f).items() if k in ("kernels", "run")}


def medians(d, path=""):
    """{dotted path: the median} of every timing summary (pet._summary's dict) in a child's result"""
    out = {}
    for k, v in d.items():
        if isinstance(v, dict):
            m = next((v[u] for u in ("median_us", "median_ms") if u in v), None)
            if m is not None:
                out[path + k] = m
            else:
                out.update(medians(v, path + k + "."))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True, help="a built checkout of the parent commit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "source_core_perf.json"))
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--merge", action="append", default=[], metavar="NAME=FILE")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("perf_source_core.py measures on the GPU: none is visible")
    trees = [("parent", os.path.abspath(a.parent)), ("new", ROOT)]
    out = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "hip": torch.version.hip, "rounds": a.rounds,
           "warmup_rounds": a.warmup, "repeats": a.repeats,
           "what": "per figure: each tree's process medians (fresh processes, the trees alternating in swapped order), and whether the "
                   "median of this tree's lies within min .. max of the parent's"}
    ok = True
    for name, tool, mode, state in STEPS:
        runs = {"parent": [], "new": []}
        for i in range(a.repeats):
            for which, tree in (trees if i % 2 == 0 else trees[::-1]):
                runs[which].append(medians(child(tool, mode, tree, state, a)))
        res = {}
        for fig in runs["parent"][0]:
            if fig.startswith("torch_") or ".torch_" in fig:                      # not this project's kernels
                continue
            p, n = [r[fig] for r in runs["parent"]], [r[fig] for r in runs["new"]]
            res[fig] = {"parent": p, "new": n, "new_median": statistics.median(n), "parent_range": [min(p), max(p)],
                        "new_inside_the_parent_range": min(p) <= statistics.median(n) <= max(p),
                        "new_not_slower_than_the_parent_range": statistics.median(n) <= max(p)}
            ok &= res[fig]["new_not_slower_than_the_parent_range"]
        out[name] = res
        print(name, {k: (round(v["new_median"], 3), [round(x, 3) for x in v["parent_range"]]) for k, v in res.items()}, file=sys.stderr, flush=True)
    for m in a.merge:
        key, path = m.split("=", 1)
        with open(path) as f:
            out[key] = json.load(f)
    out["every_figure_not_slower_than_the_parent_range"] = ok
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
