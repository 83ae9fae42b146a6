"""What shuffled env-sequence minibatches cost -> profiles/env_shuffle_perf.json.

  (a) gather    one uav_gather_rows_multi launch packing the nine arrays of a minibatch (obs, keep, act, logp, adv_n, ret, val
                [N][T].., h0, c0 [L][N][H]) of n_sel = 512 of N = 4096 envs, against `chain`: the nine torch.index_select calls
                (out= buffers allocated once, int64 index prepared outside the timed region) that produce the same tensors --
                asserted equal first.  Two shapes: the C3 minibatch (T = 128, D = 6, H = 128, L = 1) and a C5-like one (T = 256,
                D = 8, H = 256, L = 2).  HIP events around one form's work, the two forms alternating, a fresh chunk of one
                permutation per launch; `--launches` timed launches after as many warm ones.  Accepted if the gather's median is
                no larger than the chain's.  bytes (read + written) over the median is recorded beside the device's 6.3 TB/s
                copy rate for information: at 3.6 MB a launch this copy is bound by launch and memory latency, not bandwidth.
  (b) iteration train_iteration() at the C3 shape (4096 envs x 128 steps, LSTM h = 128, curriculum on) with num_minibatches = 8,
                shuffle_envs on and off, each in fresh processes (`--repeats` of them per variant, the variants alternating),
                HIP events around every iteration, `--iterations` timed ones after `--warmup`; with --parent-root (a built
                checkout of the parent commit) the unshuffled iteration of that tree the same way.  Accepted if
                  * the unshuffled median is within run-to-run spread of the parent's: |difference of the medians| <= the
                    larger of the two p10 .. p90 widths (that path is unchanged; without --parent-root this is not decided);
                  * (shuffled - unshuffled median) / (epochs x num_minibatches optimiser steps) <= the chain's median of (a)
                    at the C3 shape: the packed route must not cost more per step than the route it replaces.

The parent process never opens the GPU; every measurement is a child process of its own.

    python tools/perf_env_shuffle.py [--out profiles/env_shuffle_perf.json] [--launches 60] [--parent-root DIR]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_ENV, N_SEL, M, EPOCHS = 4096, 512, 8, 5
SHAPES = {"c3": dict(T=128, D=6, H=128, L=1), "c5_like": dict(T=256, D=8, H=256, L=2)}
DEV = "cuda:0"
COPY_RATE_TBS = 6.3


def _spread(ms):
    ms = sorted(ms)
    return {"median_ms": statistics.median(ms), "min_ms": ms[0], "max_ms": ms[-1], "p10_ms": ms[len(ms) // 10],
            "p90_ms": ms[(9 * len(ms)) // 10], "n": len(ms)}


def _event_ms(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def part_gather(launches):
    import torch
    from uavppo import ops
    out = {}
    for name, s in SHAPES.items():
        T, D, H, L = s["T"], s["D"], s["H"], s["L"]
        g = torch.Generator(device=DEV).manual_seed(1)
        f = lambda *sh: torch.randn(*sh, generator=g, device=DEV)
        srcs = [(f(N_ENV, T, D), 0), (f(N_ENV, T), 0), (torch.randint(0, 5, (N_ENV, T), generator=g, device=DEV, dtype=torch.int32), 0),
                (f(N_ENV, T), 0), (f(N_ENV, T), 0), (f(N_ENV, T), 0), (f(N_ENV, T), 0), (f(L, N_ENV, H), 1), (f(L, N_ENV, H), 1)]

        def like(a, rd):
            shape = list(a.shape)
            shape[rd] = N_SEL
            return torch.zeros(shape, dtype=a.dtype, device=DEV)
        packed = [like(a, rd) for a, rd in srcs]
        chained = [like(a, rd) for a, rd in srcs]
        plan = ops.GatherPlan([(a, d, rd) for (a, rd), d in zip(srcs, packed)])
        perm = torch.randperm(N_ENV, generator=g, device=DEV)
        idx64 = [c.contiguous() for c in perm.split(N_SEL)]
        idx32 = [c.to(torch.int32).contiguous() for c in idx64]

        def gather(i):
            ops.gather_rows_multi(idx32[i], plan)

        def chain(i):
            for (a, rd), d in zip(srcs, chained):
                torch.index_select(a, rd, idx64[i], out=d)

        fns = {"gather": gather, "chain": chain}
        same = True
        for i in range(len(idx32)):
            gather(i)
            chain(i)
            torch.cuda.synchronize()
            same = same and all(torch.equal(p, c) for p, c in zip(packed, chained))
        ms = {k: [] for k in fns}
        for timed in (False, True):                  # as many warm launches as timed ones, in the same order
            for n in range(launches):
                for k, fn in fns.items():
                    t = _event_ms(lambda: fn(n % len(idx32)))
                    if timed:
                        ms[k].append(t)
        payload = sum(d.numel() * d.element_size() for d in packed)
        r = {"shape": dict(s, envs=N_ENV, n_sel=N_SEL), "arrays": len(srcs), "payload_bytes": payload,
             "gather_equals_chain_bitwise": bool(same)}
        r.update({k: _spread(v) for k, v in ms.items()})
        r["gather_over_chain_medians"] = r["gather"]["median_ms"] / r["chain"]["median_ms"]
        r["gather_read_plus_written_tb_per_s"] = 2 * payload / (r["gather"]["median_ms"] * 1e-3) / 1e12
        r["device_copy_rate_tb_per_s_for_information"] = COPY_RATE_TBS
        r["accepted_gather_le_chain"] = r["gather"]["median_ms"] <= r["chain"]["median_ms"]
        out[name] = r
    out["device"] = torch.cuda.get_device_name(0)
    return out


def part_iteration(shuffle, warmup, iterations):
    import torch
    from uavppo.trainer import VecPPOTrainer
    kw = {"shuffle_envs": True} if shuffle else {}           # (a parent checkout does not know the keyword)
    tr = VecPPOTrainer(N_ENV, SHAPES["c3"]["T"], "lstm", hidden=SHAPES["c3"]["H"], device=DEV, seed=1, lr=3e-4, num_minibatches=M,
                       use_curriculum=True, **kw)
    assert tr.hp["epochs"] == EPOCHS
    for _ in range(warmup):
        tr.train_iteration()
    torch.cuda.synchronize()
    evs = [torch.cuda.Event(enable_timing=True) for _ in range(iterations + 1)]
    evs[0].record()
    for i in range(iterations):
        tr.train_iteration()
        evs[i + 1].record()
    torch.cuda.synchronize()
    tr.losses()                                              # raises on NaN
    return {"ms": [evs[i].elapsed_time(evs[i + 1]) for i in range(iterations)]}


def _child(root, *args):
    """One measurement in a fresh process that imports the package of `root`; its last output line is the JSON result."""
    cmd = [sys.executable, os.path.abspath(__file__), "--root", root] + [str(a) for a in args]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise SystemExit(f"{' '.join(cmd)} failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "env_shuffle_perf.json"))
    ap.add_argument("--launches", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=15)
    ap.add_argument("--iterations", type=int, default=60)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--root", default=ROOT, help=argparse.SUPPRESS)
    ap.add_argument("--part", choices=("gather", "iteration"), default=None, help=argparse.SUPPRESS)
    ap.add_argument("--shuffle", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.part is not None:
        sys.path[:0] = [a.root, os.path.join(a.root, "uav-wrf-les-ppo-lstm_amd")]
        res = part_gather(a.launches) if a.part == "gather" else part_iteration(bool(a.shuffle), a.warmup, a.iterations)
        print(json.dumps(res), flush=True)
        return
    out = {"gather": _child(ROOT, "--part", "gather", "--launches", a.launches)}
    print("gather:", {s: out["gather"][s]["gather_over_chain_medians"] for s in SHAPES}, file=sys.stderr, flush=True)
    variants = {"unshuffled": (ROOT, 0), "shuffled": (ROOT, 1)}
    if a.parent_root:
        variants["parent_unshuffled"] = (os.path.abspath(a.parent_root), 0)
    ms = {k: [] for k in variants}
    per_process = {k: [] for k in variants}
    for _ in range(a.repeats):
        for k, (root, shuffle) in variants.items():
            got = _child(root, "--part", "iteration", "--shuffle", shuffle, "--warmup", a.warmup, "--iterations", a.iterations)["ms"]
            print(f"{k}: median {statistics.median(got):.3f} ms over {len(got)} iterations", file=sys.stderr, flush=True)
            ms[k] += got
            per_process[k].append(statistics.median(got))
    it = {"shape": dict(SHAPES["c3"], envs=N_ENV, num_minibatches=M, epochs=EPOCHS, policy="lstm", curriculum=True),
          "warmup": a.warmup, "iterations_per_process": a.iterations, "processes_per_variant": a.repeats,
          "process_medians_ms": per_process}
    it.update({k: _spread(v) for k, v in ms.items()})
    steps = EPOCHS * M
    chain_ms = out["gather"]["c3"]["chain"]["median_ms"]
    excess = it["shuffled"]["median_ms"] - it["unshuffled"]["median_ms"]
    it["optimiser_steps_per_iteration"] = steps
    it["shuffled_excess_ms"] = excess
    it["shuffled_excess_per_step_us"] = 1e3 * excess / steps
    it["chain_per_step_us"] = 1e3 * chain_ms
    it["accepted_excess_per_step_le_chain"] = excess / steps <= chain_ms
    if a.parent_root:
        width = lambda s: s["p90_ms"] - s["p10_ms"]
        it["run_to_run_spread_ms"] = max(width(it["unshuffled"]), width(it["parent_unshuffled"]))
        it["unshuffled_minus_parent_ms"] = it["unshuffled"]["median_ms"] - it["parent_unshuffled"]["median_ms"]
        it["accepted_unshuffled_within_spread_of_parent"] = abs(it["unshuffled_minus_parent_ms"]) <= it["run_to_run_spread_ms"]
    else:
        it["accepted_unshuffled_within_spread_of_parent"] = None
    out["iteration"] = it
    out["device"] = out["gather"].pop("device")
    ok = (all(out["gather"][s]["accepted_gather_le_chain"] and out["gather"][s]["gather_equals_chain_bitwise"] for s in SHAPES)
          and it["accepted_excess_per_step_le_chain"] and it["accepted_unshuffled_within_spread_of_parent"] is not False)
    out["accepted"] = bool(ok)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)
    if not ok:
        raise SystemExit("acceptance failed")


if __name__ == "__main__":
    main()
