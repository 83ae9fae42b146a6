"""What the source estimate costs -> profiles/source_fit_perf.json.

    kernels    us per call of uav_source_moments (a 1024 x 250 x 6 chunk of records of E3's formula, walkers around the source),
               uav_source_solve and uav_source_summary (1024 envs) alone, each between two HIP events; and the same moments as ONE
               torch masked reduction over the same records (elementwise torch ops and a sum over the steps; f64, no chunk state).
    run        one EvalTracker.run() (1024 evaluation envs, the env's own step limit, LSTM h = 128) with the option on and off,
               HIP events, one process each.
    iteration  ms per train_iteration() at C2 (256 x 64, LSTM h = 64) and C3 (4096 x 128, LSTM h = 128) with the option off against
               --parent PATH (a built checkout of the parent commit): fresh processes that alternate, as tools/perf_eval_track.py does
               (its children are used).
    launches   with --parent: kernel names and call counts of ten C2 iterations with the option off, one rocprofv3 run per tree:
               the tables must be equal.

    python tools/perf_source_fit.py [--parent PATH] [--what kernels,run,iteration,launches] [--out profiles/source_fit_perf.json]
                                    [--rounds 20] [--warmup 5] [--repeats 3]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import perf_eval_track as pet  # noqa: E402

DEV = pet.DEV
N, K, D = 1024, 250, 6


def _records(torch):
    """flags / obs / pos of N x K records on the device: a source per env, positions 0.5 .. 3.5 sigma around it, E3's formula at the
    position's cell, an end by bit0 somewhere in the last fifth of a third of the envs."""
    g = torch.Generator(device=DEV).manual_seed(1)
    u = lambda *s: torch.rand(*s, device=DEV, generator=g, dtype=torch.float64)
    sigma = 500.0 / 16.0
    src = 150.0 + 200.0 * u(N, 2)
    rad, ang = sigma * (0.5 + 3.0 * u(N, K)), 6.283185307179586 * u(N, K)
    pos = (src[:, None, :] + torch.stack([rad * torch.cos(ang), rad * torch.sin(ang)], 2)).to(torch.float32)
    cell = pos.clamp(0.0, 499.0).to(torch.int32).to(torch.float64)
    d2 = ((cell - src[:, None, :]) ** 2).sum(2)
    tke = 6.0 * u(N, K)
    conc = (100.0 * torch.exp(-d2 / (2.0 * sigma * sigma)) + tke).clamp(0.0, 100.0)
    obs = torch.rand(N, K, D, device=DEV, generator=g)
    obs[:, :, 2] = (conc / 100.0).to(torch.float32)
    obs[:, :, 3] = (tke / 9.0).to(torch.float32)
    flags = torch.zeros(N, K, dtype=torch.uint8, device=DEV)
    e = torch.arange(0, N, 3, device=DEV)
    flags[e, K - 1 - (e % (K // 5))] = 1
    return {"flags": flags, "obs": obs.contiguous(), "pos": pos.contiguous()}, src.contiguous()


def _torch_moments(torch, recs, floor=1.0):
    """The moments of uav_source_moments as one masked reduction in torch (f64): [N, 15]"""
    f, obs, pos = recs["flags"], recs["obs"], recs["pos"]
    k = f.shape[1]
    idx = torch.arange(k, device=f.device)
    end = ((f & 4) == 0) & ((f & 9) != 0)
    first = torch.where(end.any(1), end.to(torch.int32).argmax(1), torch.full_like(idx[:1], k - 1).expand(f.shape[0]))
    take = ((f & 4) == 0) & (idx[None, :] <= first[:, None])
    o2 = obs[:, :, 2]
    b = 100.0 * o2.to(torch.float64) - 9.0 * obs[:, :, 3].to(torch.float64)
    used = take & (b > floor) & (o2 < 1.0)
    cell = pos.clamp(0.0, 499.0).to(torch.int32).to(torch.float64)
    i0 = used.to(torch.int32).argmax(1)
    c = cell[torch.arange(f.shape[0], device=f.device), i0]
    p, q = (cell[:, :, 0] - c[:, 0:1]) / 32.0, (cell[:, :, 1] - c[:, 1:2]) / 32.0
    r = p * p + q * q
    bu = torch.where(used, b, torch.ones_like(b))
    w, lb = bu * bu, torch.log(bu)
    wp, wq, wr = w * p, w * q, w * r
    terms = torch.stack([torch.ones_like(w), w, wp, wq, wr, wp * p, wp * q, wp * r, wq * q, wq * r, wr * r, w * lb, wp * lb, wq * lb,
                         wr * lb], 2)
    return (terms * used[:, :, None]).sum(1)


def child_kernels(tree, _shape, _state, warmup, rounds):
    pet._paths(tree)
    import torch
    from uavppo import ops
    recs, src = _records(torch)
    cfg = ops.source_fit_cfg()
    z = lambda dt, *s: torch.zeros(*s, dtype=dt, device=DEV)
    state, est, status = z(torch.float64, N, ops.SRC_STATE_N), z(torch.float64, N, ops.SRC_EST_N), z(torch.uint8, N)
    sums, ended = z(torch.float64, ops.SRC_SUM_N), z(torch.uint8, N)
    ops.source_moments(recs, cfg, state, ended)
    want = _torch_moments(torch, recs)
    agree = float(((state[:, 0] - want[:, 0]).abs().max()).item()), float(((state[:, 3:17] - want[:, 1:]).abs() /
                                                                            want[:, 1:].abs().clamp(min=1e-300)).max().item())
    calls = {"uav_source_moments": lambda: ops.source_moments(recs, cfg, state, ended),
             "uav_source_solve": lambda: ops.source_solve(state, cfg, est, status),
             "uav_source_summary": lambda: ops.source_summary(est, status, src, 31.25, 100.0, 5.0, sums),
             "torch_masked_reduction": lambda: _torch_moments(torch, recs)}
    us = {c: [] for c in calls}
    for r in range(warmup + rounds):
        state.zero_()
        ops.source_moments(recs, cfg, state, ended)
        for c, f in calls.items():
            us[c].append(pet._timed(torch, f) * 1e3)
    out = {c: pet._summary(v[warmup:], "us") for c, v in us.items()}
    out["chunk"] = [N, K, D]
    out["fitted_envs"] = int((status == 0).sum().item())
    out["records_used_per_env_mean"] = float(want[:, 0].mean().item())
    out["torch_against_kernel"] = {"count_max_abs_difference": agree[0], "moments_max_relative_difference": agree[1]}
    print(json.dumps(out), flush=True)


def child_run(tree, _shape, state, warmup, rounds):
    pet._paths(tree)
    import torch
    from uavppo import ops
    from uavppo.trainer import VecPPOTrainer
    tr = VecPPOTrainer(64, 16, "lstm", hidden=128, device=DEV, seed=1, eval_every=1, eval_envs=N, eval_source_fit=state == "on")
    t = tr.eval_tracker
    ms = []
    for r in range(warmup + rounds):
        ms.append(pet._timed(torch, lambda: t.run(r)))
        t.curve()
    rows = t.curve(wait=True)
    out = {"route": t.route, "limit": t.limit, "chunk": t.chunk, "device": pet._summary(ms[warmup:], "ms"),
           "successes": int(rows[-1]["sums"][1]), "steps": int(rows[-1]["sums"][2])}
    if state == "on":
        out["source_sums"] = dict(zip(ops.SRC_SUM_NAMES, [float(v) for v in rows[-1]["source"]]))
    print(json.dumps(out), flush=True)


CHILDREN = {"kernels": child_kernels, "run": child_run}


def run_child(mode, state, a):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", mode, ROOT, "c3", state, "--warmup", str(a.warmup), "--rounds", str(a.rounds)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if r.returncode != 0:                               # nothing more is started on the device after a failure
        raise SystemExit(f"{cmd}: exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}")
    return pet.last_json(r.stdout)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", nargs=4, metavar=("MODE", "TREE", "SHAPE", "STATE"))
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--what", default="kernels,run,iteration,launches")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "source_fit_perf.json"))
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    if a.child:
        return CHILDREN[a.child[0]](a.child[1], a.child[2], a.child[3], a.warmup, a.rounds)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("perf_source_fit.py measures on the GPU: none is visible")
    what = a.what.split(",")
    parent = os.path.abspath(a.parent) if a.parent else None
    out = {"device": torch.cuda.get_device_name(0), "compute_units": torch.cuda.get_device_properties(0).multi_processor_count,
           "torch": torch.__version__, "hip": torch.version.hip, "rounds": a.rounds, "warmup_rounds": a.warmup, "ranks": 1,
           "parent_tree_measured": bool(parent),
           "not_measured": "fit rates of trained policies at the curriculum's radii; several ranks"}

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")

    if "kernels" in what:
        out["kernels"] = {"what": "us per call alone, HIP events around one call, one process", "calls": run_child("kernels", "off", a)}
        save()
    if "run" in what:
        res = {s: run_child("run", s, a) for s in ("off", "on")}
        res["added_ms"] = res["on"]["device"]["median_ms"] - res["off"]["device"]["median_ms"]
        res["same_successes_and_steps"] = all(res["on"][k] == res["off"][k] for k in ("successes", "steps"))
        out["run"] = dict(res, what=f"one EvalTracker.run() of {N} envs, LSTM h = 128, the option off and on; one process each")
        print("run", res["off"]["device"]["median_ms"], "->", res["on"]["device"]["median_ms"], "ms", file=sys.stderr, flush=True)
        save()
    for shape in (pet.SHAPES if "iteration" in what else []):
        runs = {k: [] for k in (["parent"] if parent else []) + ["off"]}
        for i in range(a.repeats):
            pair = ([("parent", parent)] if parent else []) + [("off", ROOT)]
            for name, tree in (pair if i % 2 == 0 else pair[::-1]):      # parent, off | off, parent | ...: neither is always first
                runs[name].append(pet.last_json(pet.run_child("iteration", tree, shape, "off", a)))
        med = {k: [r["median_ms"] for r in v] for k, v in runs.items()}
        res = {"what": "ms per train_iteration(), the option off; one fresh process per entry of `runs`", "shape": pet.SHAPES[shape],
               "runs": runs, "median_of_process_medians_ms": {k: statistics.median(v) for k, v in med.items()}}
        if parent:
            res["parent_range_ms"] = [min(med["parent"]), max(med["parent"])]
        out.setdefault("iteration", {})[shape] = res
        print(shape, {k: [round(x, 4) for x in v] for k, v in med.items()}, file=sys.stderr, flush=True)
        save()
    ok = True
    if "launches" in what and parent:
        tables = {"parent": pet.launch_table(parent, a), "off": pet.launch_table(ROOT, a)}
        same = tables["parent"] == tables["off"]
        out["launches"] = {"shape": pet.SHAPES["c2"], "iterations": pet.TRACE_ITERS, "kernels": len(tables["off"]),
                           "calls": sum(tables["off"].values()), "off_equals_parent": same,
                           "off_vs_parent": {n: [tables["parent"].get(n, 0), tables["off"].get(n, 0)]
                                             for n in sorted(set(tables["parent"]) | set(tables["off"]))
                                             if tables["parent"].get(n, 0) != tables["off"].get(n, 0)}}
        print("launch tables", "equal" if same else "DIFFERENT", out["launches"]["off_vs_parent"], file=sys.stderr, flush=True)
        ok &= same
        save()
    print(json.dumps(out), flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
