"""What the fused kernels buy a trend-observation policy, and what the trend form costs the kernel -> profiles/trend_fused_perf.json.

Shape: 4096 envs x 128 steps, one LSTM layer of h = 128, trend_k = 2 (obs_dim 8), procedural fields.

  (a) collect() on uav_rollout (TREND form, stash / y / heads written for epoch 0) against _collect_stepwise_lstm on the SAME
      trainer -- what such a policy ran on before -- alternating in blocks, HIP events around each call;
      train_iteration() with the fused rollout and the adopted epoch 0 against a twin trainer whose collect() is the step-wise
      rollout (so every epoch runs its forward pass), A/B/A/B in blocks, wall clock between device synchronisations;
      evaluate(fused=True) against evaluate(fused=False), 1000 envs, 300-step cap, alternating, wall clock between
      synchronisations;
  (b) one uav_rollout launch with trend_k = 0, 1, 2, without and with stash / y_out / heads, round-robin in blocks, HIP events:
      the k > 0 forms do the same MFMA work (K = 8 either way) and store 4 k more bytes per env-step, 4 H more with the stash.

Every figure is the median of `--launches` warm launches with min / max / p10 / p90.  The file is rewritten after every
finished measurement, so a run that ends early leaves what it had measured.

    python tools/perf_trend_rollout.py [--out profiles/trend_fused_perf.json] [--launches 30] [--block 5] [--only a b]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "uav-wrf-les-ppo-lstm_amd")]

import torch  # noqa: E402

N_ENV, T, H, K = 4096, 128, 128, 2
DEV = "cuda:0"


def _spread(ms):
    ms = sorted(ms)
    return {"median_ms": statistics.median(ms), "min_ms": ms[0], "max_ms": ms[-1], "p10_ms": ms[len(ms) // 10],
            "p90_ms": ms[(9 * len(ms)) // 10], "n": len(ms)}


def _event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _wall_ms(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def _alternate(fns, launches, block, clock):
    """{name: [ms]} of `launches` calls of every fn, taken in alternating blocks of `block` after two warm calls each."""
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
    return VecPPOTrainer(N_ENV, T, "lstm", hidden=H, device=DEV, seed=1, use_curriculum=False, trend_k=k, **kw)


def _stepwise(tr):
    """collect() as it ran for this policy before the TREND kernels: the step-wise rollout (its code is unchanged)."""
    tr._rollout_forward_valid = False
    tr._state0.copy_(tr._state)
    tr._collect_stepwise_lstm(None, None)


def measure_collect(a):
    tr = _trainer(K)
    ms = _alternate({"fused": tr.collect, "stepwise": lambda: _stepwise(tr)}, a.launches, a.block, _event_ms)
    assert tr.nan_count.item() == 0
    row = {k: _spread(v) for k, v in ms.items()}
    row["stepwise_over_fused_medians"] = row["stepwise"]["median_ms"] / row["fused"]["median_ms"]
    row["stepwise_ms_per_step"] = row["stepwise"]["median_ms"] / T
    return row


def measure_iteration(a):
    fused, step = _trainer(K), _trainer(K)
    step.collect = lambda forced_act=None, noise=None: _stepwise(step)          # twin trainer: step-wise rollout, no adoption
    ms = _alternate({"fused_adopted": fused.train_iteration, "stepwise_recomputed": step.train_iteration}, a.launches, a.block,
                    _wall_ms)
    assert all(map(lambda v: v == v, fused.losses() + step.losses()))
    row = {k: _spread(v) for k, v in ms.items()}
    row["epochs"] = fused.hp["epochs"]
    row["stepwise_over_fused_medians"] = row["stepwise_recomputed"]["median_ms"] / row["fused_adopted"]["median_ms"]
    return row


def measure_eval(a):
    import evaluate_with_lstm as ev
    from uavppo.policy import LSTMActorCritic
    from uavppo.vec_env import VecMethaneEnv
    n, cap = 1000, 300
    pol = LSTMActorCritic(6 + K, H, 1, device=DEV, seed=1)
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


def measure_kernel(a):
    from uavppo import ops
    trs = {k: _trainer(k) for k in (0, 1, 2)}

    def launch(tr, stash):
        def fn():
            ops.rollout_lstm(tr.env_state, tr.N, tr.env_cfg(), tr.policy.flat, H, T, tr.iteration, tr.cur_obs, tr.h[0], tr.c[0],
                             tr.buf, last_val=tr.last_val, nan_count=tr.nan_count, stash=tr.work["stash0"] if stash else None,
                             y=tr.work["y0"] if stash else None, heads=tr.work["heads"] if stash else None)
        return fn

    fns = {f"k{k}_{'stash' if s else 'lean'}": launch(trs[k], s) for s in (False, True) for k in (0, 1, 2)}
    ms = _alternate(fns, a.launches, a.block, _event_ms)
    row = {k: _spread(v) for k, v in ms.items()}
    for s in ("lean", "stash"):
        for k in (1, 2):
            row[f"k{k}_over_k0_{s}"] = row[f"k{k}_{s}"]["median_ms"] / row[f"k0_{s}"]["median_ms"]
        # bytes the kernel writes per env-step: obs 4 (6 + k), act / rew / val / logp / done 20, keep 4, flags 1; with the stash
        # 6 H gate / c_prev columns (5 H at k = 0: no h_prev slot), y H, heads 24
        row[f"bytes_per_env_step_{s}"] = {f"k{k}": 4 * (6 + k) + 25 + (4 * ((6 if k else 5) * H + H) + 24 if s == "stash" else 0)
                                          for k in (0, 1, 2)}
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trend_fused_perf.json"))
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--block", type=int, default=5)
    ap.add_argument("--only", nargs="+", choices=("collect", "iteration", "eval", "kernel"), default=None)
    a = ap.parse_args()
    out = {"shape": {"envs": N_ENV, "T": T, "hidden": H, "trend_k": K, "fields": "procedural"},
           "device": torch.cuda.get_device_name(0), "launches": a.launches, "block": a.block}
    if os.path.exists(a.out) and a.only:
        with open(a.out) as f:
            out = dict(json.load(f), **out)
    for name, fn in (("collect", measure_collect), ("iteration", measure_iteration), ("eval", measure_eval),
                     ("kernel", measure_kernel)):
        if a.only and name not in a.only:
            continue
        out[name] = fn(a)
        torch.cuda.empty_cache()
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
        print(json.dumps({name: out[name]}), flush=True)


if __name__ == "__main__":
    main()
