"""What the estimator's stop rule costs -> profiles/source_stop_perf.json.

    kernels    us per call of uav_source_stop_scan on a 1024 x 50 x 6 and a 1024 x 250 x 6 chunk of records (walkers around the source,
               E3's formula), between two HIP events: with a rule that cannot fire (every record is scanned and solved) and with the
               default rule (the scan ends at the hit).  Beside it the same prefix moments and per-record solves as batched torch
               operations (a cumsum over the steps, the scaled Cholesky written out elementwise over [N, k]): what one would write
               without the kernel.  Its estimates are checked against the kernel's.
    run        one EvalTracker.run() (1024 evaluation envs, the env's own step limit, LSTM h = 128) with the option off, with
               source_fit, with source_stop, and with a source_stop that cannot fire; HIP events, one process each.
    iteration  ms per train_iteration() at C2 (256 x 64, LSTM h = 64) and C3 (4096 x 128, LSTM h = 128) with the option off against
               --parent PATH (a built checkout of the parent commit): fresh processes that alternate in swapped order.
    launches   with --parent: kernel names and call counts of ten C2 iterations with the option off, one rocprofv3 run per tree:
               the tables must be equal.
    resources  VGPRs, spills and occupancy of source_stop_kernel as the compiler reports them (no GPU needed).

    python tools/perf_source_stop.py [--parent PATH] [--what kernels,run,iteration,launches,resources]
                                     [--out profiles/source_stop_perf.json] [--rounds 20] [--warmup 5] [--repeats 3]
A run of some of the steps keeps the others' entries of an existing --out file.
"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import perf_eval_track as pet  # noqa: E402

DEV = pet.DEV
N, D = 1024, 6
CHUNKS = (50, 250)
NEVER = 1 << 30


def _records(torch, k):
    """flags / obs / pos of N x k records on the device: a source per env, positions 0.5 .. 3.5 sigma around it, E3's formula at the
    position's cell, an end by bit0 somewhere in the last fifth of a third of the envs (tools/perf_source_fit.py's records)."""
    g = torch.Generator(device=DEV).manual_seed(1)
    u = lambda *s: torch.rand(*s, device=DEV, generator=g, dtype=torch.float64)
    sigma = 500.0 / 16.0
    src = 150.0 + 200.0 * u(N, 2)
    rad, ang = sigma * (0.5 + 3.0 * u(N, k)), 6.283185307179586 * u(N, k)
    pos = (src[:, None, :] + torch.stack([rad * torch.cos(ang), rad * torch.sin(ang)], 2)).to(torch.float32)
    cell = pos.clamp(0.0, 499.0).to(torch.int32).to(torch.float64)
    d2 = ((cell - src[:, None, :]) ** 2).sum(2)
    tke = 6.0 * u(N, k)
    conc = (100.0 * torch.exp(-d2 / (2.0 * sigma * sigma)) + tke).clamp(0.0, 100.0)
    obs = torch.rand(N, k, D, device=DEV, generator=g)
    obs[:, :, 2] = (conc / 100.0).to(torch.float32)
    obs[:, :, 3] = (tke / 9.0).to(torch.float32)
    flags = torch.zeros(N, k, dtype=torch.uint8, device=DEV)
    e = torch.arange(0, N, 3, device=DEV)
    flags[e, k - 1 - (e % (k // 5))] = 1
    return {"flags": flags, "obs": obs.contiguous(), "pos": pos.contiguous()}


def _torch_estimates(torch, recs, floor=1.0, min_samples=5.0, min_pivot=1e-6):
    """Every record's estimate as batched torch operations (f64): the masked terms, a cumsum over the steps, the scaled Cholesky of
    source_fit.coefficients elementwise over [N, k] -> (mu [N, k, 2], fitted bool [N, k])."""
    f, obs, pos = recs["flags"], recs["obs"], recs["pos"]
    n, k = f.shape
    idx = torch.arange(k, device=f.device)
    end = ((f & 4) == 0) & ((f & 9) != 0)
    first = torch.where(end.any(1), end.to(torch.int32).argmax(1), torch.full_like(idx[:1], k - 1).expand(n))
    take = ((f & 4) == 0) & (idx[None, :] <= first[:, None])
    o2 = obs[:, :, 2]
    b = 100.0 * o2.to(torch.float64) - 9.0 * obs[:, :, 3].to(torch.float64)
    used = take & (b > floor) & (o2 < 1.0)
    cell = pos.clamp(0.0, 499.0).to(torch.int32).to(torch.float64)
    c = cell[torch.arange(n, device=f.device), used.to(torch.int32).argmax(1)]
    p, q = (cell[:, :, 0] - c[:, 0:1]) / 32.0, (cell[:, :, 1] - c[:, 1:2]) / 32.0
    phi = [torch.ones_like(p), p, q, p * p + q * q]
    bu = torch.where(used, b, torch.ones_like(b))
    w, lb = bu * bu * used, torch.log(bu)
    count = used.to(torch.float64).cumsum(1)
    A = {(i, j): (w * phi[i] * phi[j]).cumsum(1) for i in range(4) for j in range(i, 4)}
    g = [(w * phi[i] * lb).cumsum(1) for i in range(4)]
    d = [torch.sqrt(A[(j, j)]) for j in range(4)]
    S = {(i, j): A[(j, i)] / (d[i] * d[j]) for i in range(4) for j in range(i + 1)}
    L, ok = {}, count >= min_samples
    for j in range(4):
        s = S[(j, j)]
        for m in range(j):
            s = s - L[(j, m)] * L[(j, m)]
        ok = ok & torch.isfinite(s) & (s >= min_pivot)
        L[(j, j)] = torch.sqrt(s)
        for i in range(j + 1, 4):
            t = S[(i, j)]
            for m in range(j):
                t = t - L[(i, m)] * L[(j, m)]
            L[(i, j)] = t / L[(j, j)]
    z, x = [None] * 4, [None] * 4
    for j in range(4):
        t = g[j] / d[j]
        for m in range(j):
            t = t - L[(j, m)] * z[m]
        z[j] = t / L[(j, j)]
    for j in (3, 2, 1, 0):
        t = z[j]
        for m in range(j + 1, 4):
            t = t - L[(m, j)] * x[m]
        x[j] = t / L[(j, j)]
    a = [x[j] / d[j] for j in range(4)]
    s2 = -1.0 / (2.0 * a[3])
    fitted = take & ok & torch.isfinite(a[0]) & torch.isfinite(a[1]) & torch.isfinite(a[2]) & (a[3] < 0.0) & torch.isfinite(s2)
    mu = torch.stack([c[:, 0:1] + 32.0 * a[1] * s2, c[:, 1:2] + 32.0 * a[2] * s2], 2)
    return mu, fitted


def child_kernels(tree, _shape, _state, warmup, rounds):
    pet._paths(tree)
    import torch
    from uavppo import ops
    out = {}
    for k in CHUNKS:
        recs = _records(torch, k)
        flags0 = recs["flags"].clone()
        fit = ops.source_fit_cfg()
        z = lambda dt, *s: torch.zeros(*s, dtype=dt, device=DEV)
        state, first, ended = z(torch.float64, N, ops.SRC_STOP_STATE_N), z(torch.int32, N), z(torch.uint8, N)
        mu, status = z(torch.float64, N, k, 2), z(torch.uint8, N, k)
        never, rule = ops.source_stop_cfg(patience=NEVER), ops.source_stop_cfg()
        ops.source_stop_scan(recs, 0, fit, never, state, first, ended, None, mu, status, mark=False)
        tmu, tfit = _torch_estimates(torch, recs)
        kfit = status == 0
        agree = {"fitted_records_kernel": int(kfit.sum().item()), "fitted_records_torch": int(tfit.sum().item()),
                 "fitted_in_one_only": int((kfit != tfit).sum().item()),
                 "mu_max_abs_difference_cells": float((mu - tmu)[kfit & tfit].abs().max().item())}
        agree["within_1e-6_cells"] = agree["mu_max_abs_difference_cells"] <= 1e-6

        def scan(cfg, per_record):
            """the launch to time; the state is zeroed and the flags are restored in front of it, outside the events"""
            state.zero_()
            recs["flags"].copy_(flags0)
            return lambda: ops.source_stop_scan(recs, 0, fit, cfg, state, first, ended, None, mu if per_record else None,
                                                status if per_record else None, mark=True)

        calls = {"uav_source_stop_scan_cannot_fire": lambda: scan(never, False),
                 "uav_source_stop_scan_default_rule": lambda: scan(rule, False),
                 "uav_source_stop_scan_cannot_fire_per_record_outputs": lambda: scan(never, True),
                 "torch_cumsum_and_elementwise_cholesky": lambda: lambda: _torch_estimates(torch, recs)}
        us = {c: [] for c in calls}
        for r in range(warmup + rounds):
            for c, prepare in calls.items():
                us[c].append(pet._timed(torch, prepare()) * 1e3)
        res = {c: pet._summary(v[warmup:], "us") for c, v in us.items()}
        res["chunk"] = [N, k, D]
        scan(rule, False)()
        res["envs_stopped_by_the_default_rule"] = int((first >= 0).sum().item())
        res["torch_against_kernel"] = agree
        res["kernel_faster_than_torch"] = res["uav_source_stop_scan_cannot_fire"]["median_us"] < res["torch_cumsum_and_elementwise_cholesky"]["median_us"]
        out[f"{N}x{k}x{D}"] = res
    print(json.dumps(out), flush=True)


RUN_STATES = {"off": {}, "source_fit": dict(eval_source_fit=True), "source_stop": dict(eval_source_stop=True),
              "source_stop_cannot_fire": dict(eval_source_stop={"patience": NEVER})}


def child_run(tree, _shape, state, warmup, rounds):
    pet._paths(tree)
    import torch
    from uavppo import ops
    from uavppo.trainer import VecPPOTrainer
    tr = VecPPOTrainer(64, 16, "lstm", hidden=128, device=DEV, seed=1, eval_every=1, eval_envs=N, **RUN_STATES[state])
    t = tr.eval_tracker
    ms = []
    for r in range(warmup + rounds):
        ms.append(pet._timed(torch, lambda: t.run(r)))
        t.curve()
    rows = t.curve(wait=True)
    out = {"route": t.route, "limit": t.limit, "chunk": t.chunk, "radius": float(t.env.current_radius),
           "device": pet._summary(ms[warmup:], "ms"), "successes": int(rows[-1]["sums"][1]), "steps": int(rows[-1]["sums"][2])}
    if "source" in rows[-1]:
        out["source_sums"] = dict(zip(ops.SRC_SUM_NAMES, [float(v) for v in rows[-1]["source"]]))
    if "stopped" in rows[-1]:
        out["stopped_by_the_rule"] = rows[-1]["stopped"]
    print(json.dumps(out), flush=True)


CHILDREN = {"kernels": child_kernels, "run": child_run}


def run_child(mode, state, a):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", mode, ROOT, "c3", state, "--warmup", str(a.warmup), "--rounds", str(a.rounds)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if r.returncode != 0:                               # nothing more is started on the device after a failure
        raise SystemExit(f"{cmd}: exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}")
    return pet.last_json(r.stdout)


def kernel_resources():
    """What the compiler reports for source_stop_kernel (gfx950, the Makefile's flags): no GPU needed."""
    csrc = os.path.join(ROOT, "uav-wrf-les-ppo-lstm_amd", "csrc")
    cmd = ["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "--cuda-device-only",
           "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(csrc, "source_fit.hip"), "-o", os.devnull]
    text = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=csrc).stderr
    out, name = {}, None
    for line in text.splitlines():
        m = re.search(r"remark: (?:Function Name: (\S+)|\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\S+))", line)
        if not m:
            continue
        if m.group(1):
            name = m.group(1)
        elif name and "source_stop_kernel" in name:
            out[m.group(2).strip()] = m.group(3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", nargs=4, metavar=("MODE", "TREE", "SHAPE", "STATE"))
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--what", default="kernels,run,iteration,launches,resources")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "source_stop_perf.json"))
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    if a.child:
        return CHILDREN[a.child[0]](a.child[1], a.child[2], a.child[3], a.warmup, a.rounds)
    what = a.what.split(",")
    parent = os.path.abspath(a.parent) if a.parent else None
    out = json.load(open(a.out)) if os.path.exists(a.out) else {}

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")

    if "resources" in what:
        out["resources"] = {"what": "source_stop_kernel as the compiler reports it for gfx950", "kernel": kernel_resources()}
        save()
    if set(what) - {"resources"}:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("perf_source_stop.py measures on the GPU: none is visible")
        out.update({"device": torch.cuda.get_device_name(0), "compute_units": torch.cuda.get_device_properties(0).multi_processor_count,
                    "torch": torch.__version__, "hip": torch.version.hip, "rounds": a.rounds, "warmup_rounds": a.warmup, "ranks": 1,
                    "not_measured": "stop rates, deviations and estimate errors of trained policies at the curriculum's radii; several "
                                    "ranks"})
    if "kernels" in what:
        out["kernels"] = {"what": "us per call alone, HIP events around one call, one process", "chunks": run_child("kernels", "off", a)}
        save()
    if "run" in what:
        res = {s: run_child("run", s, a) for s in RUN_STATES}
        for s in RUN_STATES:
            if s != "off":
                res[s]["added_ms"] = res[s]["device"]["median_ms"] - res["off"]["device"]["median_ms"]
        out["run"] = dict(res, what=f"one EvalTracker.run() of {N} envs, LSTM h = 128, a fresh policy, the env's default radius; one "
                                    f"process each")
        print("run", {s: res[s]["device"]["median_ms"] for s in RUN_STATES}, "ms", file=sys.stderr, flush=True)
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
            res["off_inside_the_parent_range"] = min(med["parent"]) <= res["median_of_process_medians_ms"]["off"] <= max(med["parent"])
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
