"""What the behaviour-cloning kernels cost -> profiles/bc_perf.json.

(1) uav_mlp_bc_grad at 65,536 rows of a 524,288-row set (the reference's MLP, 6-256-128), contiguous and through a chunk of a
    random permutation, in both arithmetic modes, beside uav_mlp_ppo_grad / uav_mlp_ppo_grad_rows on the same rows in the same
    process, and the same cloning step through the layered path (heads() + uav_bc_loss + backward()).  The five forms alternate
    launch by launch; `--rounds` rounds of `--launches` timed launches each (after one warm round) give one median per form and
    round.  Acceptance: the cloning form's median of round medians exceeds its PPO sibling's by no more than the spread (max -
    min) of the sibling's own round medians -- the cloning loss lanes load less and compute less, the rest is the same code.
(2) One BCTrainer.epoch() on an LSTM h = 128 with 1,024 episodes of 16 .. 128 steps padded to 128, in chunks of 256 episodes:
    host clock around an epoch that ends in a synchronise.  Reported with the share of padded steps; nothing is claimed.

    python tools/perf_bc.py [--out profiles/bc_perf.json] [--launches 20] [--rounds 5]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "uav-wrf-les-ppo-lstm_amd")]

L, CHUNK = 524288, 65536
DEV = "cuda:0"


def _event_ms(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def mlp_forms(mode, launches, rounds):
    import torch
    from uavppo import ops
    from uavppo.policy import MLPActorCritic
    g = torch.Generator(device=DEV).manual_seed(1)
    pol = MLPActorCritic(6, 5, device=DEV, seed=1)
    obs = torch.rand(L, 6, generator=g, device=DEV)
    act = torch.randint(0, 5, (L,), generator=g, device=DEV).to(torch.int32)
    logp = torch.log(torch.tensor(0.2)) + 0.1 * torch.randn(L, generator=g, device=DEV)
    adv, ret, val = (torch.randn(L, generator=g, device=DEV) for _ in range(3))
    perm = torch.randperm(L, generator=g, device=DEV)
    rows = [c.contiguous() for c in perm.to(torch.int32).split(CHUNK)]
    s4, s6 = torch.zeros(4, dtype=torch.float64, device=DEV), torch.zeros(6, dtype=torch.float64, device=DEV)
    grad = torch.empty_like(pol.flat)
    inv_n = 1.0 / CHUNK
    head = lambda x: x[:CHUNK]
    stash = torch.empty(CHUNK * (2 * 256 + 2 * 128 + 2), device=DEV)
    dheads = torch.empty(CHUNK, 6, device=DEV)

    def layered(i):
        heads = pol.heads(head(obs), stash=stash)
        ops.bc_loss_heads(heads, head(act), head(ret), inv_n, 0.5, 0.01, s6, dheads)
        pol.backward(dheads)

    fns = {
        "bc_contiguous": lambda i: ops.mlp_bc_grad(pol.flat, head(obs), head(act), head(ret), inv_n, 0.5, 0.01, s6, grad),
        "ppo_contiguous": lambda i: ops.mlp_ppo_grad(pol.flat, head(obs), head(act), head(logp), head(adv), head(ret), head(val), inv_n,
                                                     0.2, 0.01, s4, grad),
        "bc_rows": lambda i: ops.mlp_bc_grad(pol.flat, obs, act, ret, inv_n, 0.5, 0.01, s6, grad, rows=rows[i]),
        "ppo_rows": lambda i: ops.mlp_ppo_grad_rows(pol.flat, obs, act, logp, adv, ret, val, rows[i], inv_n, 0.2, 0.01, s4, grad),
        "bc_layered": layered,
    }
    med = {k: [] for k in fns}
    with ops.lstm_arith(mode):
        for r in range(rounds + 1):              # round 0 warms every form
            ms = {k: [] for k in fns}
            for n in range(launches):
                for k, fn in fns.items():
                    ms[k].append(_event_ms(lambda: fn(n % len(rows))))
            if r:
                for k in fns:
                    med[k].append(statistics.median(ms[k]))
    out = {k: {"median_ms": statistics.median(v), "round_medians_ms": v, "spread_ms": max(v) - min(v)} for k, v in med.items()}
    for form in ("contiguous", "rows"):
        bc, ppo = out["bc_" + form], out["ppo_" + form]
        out[f"bc_minus_ppo_{form}_ms"] = bc["median_ms"] - ppo["median_ms"]
        out[f"accepted_{form}"] = bc["median_ms"] - ppo["median_ms"] <= ppo["spread_ms"]
    out["layered_over_fused"] = out["bc_layered"]["median_ms"] / out["bc_contiguous"]["median_ms"]
    return out


def lstm_epoch(epochs=5):
    import numpy as np
    import torch
    from uavppo.bc import BCTrainer
    from uavppo.policy import LSTMActorCritic
    rng = np.random.RandomState(1)
    lengths = rng.randint(16, 129, 1024).astype(np.int64)
    lengths[0] = 128
    M = int(lengths.sum())
    tr = BCTrainer(LSTMActorCritic(6, 128, 1, 5, DEV, seed=1), (rng.rand(M, 6).astype(np.float32), rng.randint(0, 5, M), lengths), batch=256)
    ms = []
    for e in range(2 + epochs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tr.epoch()
        torch.cuda.synchronize()
        if e >= 2:
            ms.append(1e3 * (time.perf_counter() - t0))
    return {"hidden": 128, "episodes": 1024, "padded_to": 128, "chunk_episodes": 256, "steps_per_epoch": 4, "real_steps": M,
            "padded_share": 1.0 - M / (1024 * 128), "epoch_ms": {"median": statistics.median(ms), "min": min(ms), "max": max(ms), "n": len(ms)},
            "arith": tr.guard.arith}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bc_perf.json"))
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    import torch
    out = {"shape": {"rows": L, "chunk_rows": CHUNK, "policy": "mlp 6-256-128"}, "launches": a.launches, "rounds": a.rounds,
           "device": torch.cuda.get_device_name(0)}
    for mode in ("fp16x3", "f32_mfma"):
        out[mode] = mlp_forms(mode, a.launches, a.rounds)
    out["lstm_epoch"] = lstm_epoch()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)
    if not all(out[m][f"accepted_{f}"] for m in ("fp16x3", "f32_mfma") for f in ("contiguous", "rows")):
        raise SystemExit("acceptance failed: a cloning form is slower than its PPO sibling by more than the sibling's own spread")


if __name__ == "__main__":
    main()
