"""What the fused MLP kernels buy a trend-observation MLP policy, what the width costs the kernels, and that the 6-input
path did not pay for it -> profiles/trend_mlp_fused_perf.json.

Shape: 4096 envs x 128 steps, the reference's MLP (256-128, 5 actions) with trend_k = 2 (8 inputs), procedural fields.

  (a) collect() and train_iteration() of one trainer on the fused kernels (uav_rollout policy_kind 2, uav_mlp_ppo_grad_trend)
      against its twin with fused_mlp = False -- the step-wise rollout and the layered update such a policy ran on before,
      whose code is unchanged -- alternating in blocks; HIP events around collect(), wall clock between device
      synchronisations around whole iterations;
      evaluate(fused=True) against evaluate(fused=False), 1000 envs, 300-step cap, alternating, wall clock;
  (b) one uav_rollout MLP launch and one gradient call at trend_k = 0, 1, 2, round-robin in blocks, HIP events;
  (c) the trend_k = 0 rollout launch and gradient call of this build against another build of csrc (--parent-lib, e.g. the
      parent commit's), each in a worker process of its own that loads its library through UAVPPO_LIB; this process hands
      the turn from one worker to the other block by block, so both are measured in the same minutes on the same device.
      `inside_parent_band`: this build's median lies inside (or on the fast side of) the other build's p10 .. p90.

Every figure is the median of `--launches` warm launches with min / max / p10 / p90.  The file is rewritten after every
finished measurement, so a run that ends early leaves what it had measured.

    python tools/perf_trend_mlp.py [--out profiles/trend_mlp_fused_perf.json] [--launches 30] [--block 5]
                                   [--only collect iteration eval kernel parent] [--parent-lib PATH]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "uav-wrf-les-ppo-lstm_amd")]

N_ENV, T, K = 4096, 128, 2
DEV = "cuda:0"


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


def _wall_ms(fn):
    import torch
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def _alternate(fns, launches, block, clock):
    """{name: [ms]} of `launches` calls of every fn, taken in alternating blocks of `block` after two warm calls each."""
    import torch
    for fn in fns.values():
        fn(); fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    while len(next(iter(out.values()))) < launches:
        for k, fn in fns.items():
            for _ in range(block):
                out[k].append(clock(fn))
    return out


def _trainer(k, **kw):
    from uavppo.trainer import VecPPOTrainer
    return VecPPOTrainer(N_ENV, T, "mlp", device=DEV, seed=1, use_curriculum=False, trend_k=k, **kw)


def _twins():
    fused, layered = _trainer(K), _trainer(K)
    assert fused.fused_mlp
    layered.fused_mlp = False
    return fused, layered


def measure_collect(a):
    fused, layered = _twins()
    ms = _alternate({"fused": fused.collect, "stepwise": layered.collect}, a.launches, a.block, _event_ms)
    assert fused.nan_count.item() == 0 and layered.nan_count.item() == 0
    row = {k: _spread(v) for k, v in ms.items()}
    row["stepwise_over_fused_medians"] = row["stepwise"]["median_ms"] / row["fused"]["median_ms"]
    row["stepwise_ms_per_step"] = row["stepwise"]["median_ms"] / T
    row["fused_env_steps_per_s"] = N_ENV * T / (row["fused"]["median_ms"] * 1e-3)
    return row


def measure_iteration(a):
    fused, layered = _twins()
    ms = _alternate({"fused": fused.train_iteration, "layered": layered.train_iteration}, a.launches, a.block, _wall_ms)
    assert all(map(lambda v: v == v, fused.losses() + layered.losses()))
    row = {k: _spread(v) for k, v in ms.items()}
    row["epochs"] = fused.hp["epochs"]
    row["layered_over_fused_medians"] = row["layered"]["median_ms"] / row["fused"]["median_ms"]
    return row


def measure_eval(a):
    import evaluate_with_lstm as ev
    from uavppo.policy import MLPActorCritic
    from uavppo.vec_env import VecMethaneEnv
    n, cap = 1000, 300
    pol = MLPActorCritic(6 + K, 5, device=DEV, seed=1)
    pol.views["head.weight"][:5].mul_(400.0)
    env = VecMethaneEnv(n, "v2.0", DEV, seed=7, trend_k=K)
    res = {}

    def run(fused):
        res[fused] = ev.evaluate(pol, env, max_steps=cap, fused=fused)

    ms = _alternate({"fused": lambda: run(True), "stepwise": lambda: run(False)}, max(a.launches // 3, 5), 1, _wall_ms)
    row = {k: _spread(v) for k, v in ms.items()}
    row.update(envs=n, cap=cap, env_steps=int(res[True]["steps"].sum()),
               same_steps=bool((res[True]["steps"] == res[False]["steps"]).all()),
               stepwise_over_fused_medians=row["stepwise"]["median_ms"] / row["fused"]["median_ms"],
               stepwise_ms_per_step=row["stepwise"]["median_ms"] / float(res[False]["steps"].max()))
    return row


def _kernel_fns(k, trend_entry):
    """One rollout launch and one gradient call of the trend_k = k MLP on buffers a rollout filled.  trend_entry False: the
    6-input entry points (policy_kind 0, uav_mlp_ppo_grad), which every build of csrc has."""
    import torch
    from uavppo import ops
    tr = _trainer(k)
    tr.collect()
    tr.compute_advantages()
    n = N_ENV * T
    flat = lambda t: t.reshape(-1)
    args = (tr.policy.flat, tr.buf["obs"].reshape(n, 6 + k), flat(tr.buf["act"]), flat(tr.buf["logp"]), flat(tr.adv_n), flat(tr.ret),
            flat(tr.buf["val"]), 1.0 / n, 0.2, 0.01, tr.loss_sums, tr.policy.grad)

    def rollout():
        ops.rollout_mlp(tr.env_state, tr.N, tr.env_cfg(), tr.policy.flat, T, tr.iteration, tr.cur_obs, tr.buf,
                        last_val=tr.last_val, nan_count=tr.nan_count, **({"trend": True} if trend_entry else {}))

    def grad():
        if trend_entry:
            ops.mlp_ppo_grad_trend(*args, k)
        else:
            ops.mlp_ppo_grad(*args)

    torch.cuda.synchronize()
    return rollout, grad, tr


def measure_kernel(a):
    fns, keep = {}, []
    for k in (0, 1, 2):
        rollout, grad, tr = _kernel_fns(k, True)
        fns[f"rollout_k{k}"], fns[f"grad_k{k}"] = rollout, grad
        keep.append(tr)
    ms = _alternate(fns, a.launches, a.block, _event_ms)
    row = {name: _spread(v) for name, v in ms.items()}
    for what in ("rollout", "grad"):
        for k in (1, 2):
            row[f"{what}_k{k}_over_k0"] = row[f"{what}_k{k}"]["median_ms"] / row[f"{what}_k0"]["median_ms"]
    row["rollout_env_steps_per_s"] = {f"k{k}": N_ENV * T / (row[f"rollout_k{k}"]["median_ms"] * 1e-3) for k in (0, 1, 2)}
    return row


# ---- (c): one worker process per build of the library, driven block by block over its stdin / stdout
def worker(block):
    from uavppo import _lib
    import ctypes
    probe = ctypes.CDLL(_lib.LIB_PATH)                   # an older build of csrc lacks the symbols added since
    for name in [n for n in _lib.SIGNATURES if not hasattr(probe, n)]:
        del _lib.SIGNATURES[name]
    rollout, grad, tr = _kernel_fns(0, False)
    for fn in (rollout, grad):
        fn(); fn()
    print("ready", flush=True)
    for line in sys.stdin:
        if line.strip() != "go":
            break
        print(json.dumps({"rollout": [_event_ms(rollout) for _ in range(block)], "grad": [_event_ms(grad) for _ in range(block)]}),
              flush=True)


def measure_parent(a):
    if not a.parent_lib:
        raise SystemExit("--only parent needs --parent-lib PATH (a libuavppo.so built from the csrc to compare against)")
    procs = {}
    for name, libpath in (("parent", os.path.abspath(a.parent_lib)), ("branch", None)):
        env = dict(os.environ)
        env.pop("UAVPPO_LIB", None)
        if libpath:
            env["UAVPPO_LIB"] = libpath
        procs[name] = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", "--block", str(a.block)], env=env,
                                       stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
    ms = {name: {"rollout": [], "grad": []} for name in procs}
    try:
        for name, p in procs.items():
            if p.stdout.readline().strip() != "ready":
                raise RuntimeError(f"worker {name} did not start")
        while len(ms["branch"]["rollout"]) < a.launches:
            for name, p in procs.items():
                p.stdin.write("go\n")
                p.stdin.flush()
                got = json.loads(p.stdout.readline())
                for what in got:
                    ms[name][what] += got[what]
    finally:
        for p in procs.values():
            p.stdin.close()
            p.wait(timeout=60)
    row = {"parent_lib": os.path.basename(a.parent_lib)}
    for what in ("rollout", "grad"):
        par, br = _spread(ms["parent"][what]), _spread(ms["branch"][what])
        row[what] = {"parent": par, "branch": br, "branch_over_parent_medians": br["median_ms"] / par["median_ms"],
                     "inside_parent_band": br["median_ms"] <= par["p90_ms"]}
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trend_mlp_fused_perf.json"))
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--block", type=int, default=5)
    ap.add_argument("--only", nargs="+", choices=("collect", "iteration", "eval", "kernel", "parent"), default=None)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a.block)
    import torch
    out = {"shape": {"envs": N_ENV, "T": T, "policy": "mlp 256-128", "trend_k": K, "fields": "procedural"},
           "launches": a.launches, "block": a.block}
    if os.path.exists(a.out) and a.only:
        with open(a.out) as f:
            out = dict(json.load(f), **out)
    parts = [("parent", measure_parent)] if a.parent_lib else []       # first: before this process opens the device itself
    parts += [("collect", measure_collect), ("iteration", measure_iteration), ("eval", measure_eval), ("kernel", measure_kernel)]
    for name, fn in parts:
        if a.only and name not in a.only:
            continue
        out[name] = fn(a)
        out["device"] = torch.cuda.get_device_name(0)
        torch.cuda.empty_cache()
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
        print(json.dumps({name: out[name]}), flush=True)


if __name__ == "__main__":
    main()
