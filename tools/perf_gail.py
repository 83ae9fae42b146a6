"""GAIL's cost at the C3 shape (4096 envs x 128 steps = 524,288 policy rows, a 20,000-row expert set) -> profiles/gail_perf.json.

  (a) HIP-event time of uav_disc_grad and of uav_disc_reward, warm, median of `--launches` launches with the spread;
  (b) the same discriminator step (forward, two BCELoss means, backward) and the same reward written in plain torch-ROCm on the
      same tensors in the same process -- the reference's own formulation (PPOV1.1/train_ppo_gail.py:157-175), the only
      baseline there is; (a) and (b) alternate launch by launch;
  (c) ms per GAILTrainer.train_iteration() against VecPPOTrainer.train_iteration() at C3 in one process, A/B/A/B, wall clock
      between device synchronisations.

Run without arguments it is the driver: every step that touches the GPU is a fresh child process under its own
`timeout -k 10`, and the steps are chained (a step that fails ends the run).  `--step kernels|loop` is one such child.

    python tools/perf_gail.py [--out profiles/gail_perf.json] [--launches 30] [--iters 40]
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
N_ENV, T, N_EXPERT, OD, NA = 4096, 128, 20000, 6, 5


def _spread(ms):
    ms = sorted(ms)
    return {"median_ms": statistics.median(ms), "min_ms": ms[0], "max_ms": ms[-1], "p10_ms": ms[len(ms) // 10],
            "p90_ms": ms[(9 * len(ms)) // 10], "n": len(ms)}


def step_kernels(launches):
    import torch
    import torch.nn as nn
    from uavppo import ops
    from uavppo.gail import Discriminator
    dev = "cuda:0"
    g = torch.Generator().manual_seed(0)
    n_p = N_ENV * T
    obs_e, act_e = torch.rand(N_EXPERT, OD, generator=g).to(dev), torch.randint(0, NA, (N_EXPERT,), generator=g).to(dev, torch.int32)
    obs_p, act_p = torch.rand(n_p, OD, generator=g).to(dev), torch.randint(0, NA, (n_p,), generator=g).to(dev, torch.int32)
    rew = torch.randn(n_p, generator=g).to(dev)
    disc = Discriminator(OD, NA, dev, seed=1)
    sums, grad, out = torch.zeros(4, dtype=torch.float64, device=dev), torch.zeros_like(disc.flat), torch.empty_like(rew)
    # the reference's formulation on the same tensors: one-hot rows built once outside the timed region (the reference builds
    # them per step on the host), nn.Sequential + two nn.BCELoss means + backward; the reward as env + coef * softplus(logit)
    net = nn.Sequential(nn.Linear(OD + NA, 128), nn.ReLU(), nn.Linear(128, 1), nn.Sigmoid()).to(dev)
    net.load_state_dict({k[4:]: v for k, v in disc.state_dict().items()})
    sa_e = torch.cat([obs_e, nn.functional.one_hot(act_e.long(), NA).float()], 1)
    sa_p = torch.cat([obs_p, nn.functional.one_hot(act_p.long(), NA).float()], 1)
    bce = nn.BCELoss()

    def hip_grad():
        ops.disc_grad(disc.flat, obs_e, act_e, obs_p, act_p, NA, loss_sums=sums, grad=grad)

    def torch_grad():
        for p in net.parameters():
            p.grad = None
        de, dp = net(sa_e), net(sa_p)
        (bce(de, torch.ones_like(de)) + bce(dp, torch.zeros_like(dp))).backward()

    def hip_reward():
        ops.disc_reward(disc.flat, obs_p, act_p, NA, 0.5, 1.0, rew_env=rew, out=out)

    def torch_reward():
        with torch.no_grad():
            return rew + 0.5 * nn.functional.softplus(net[:3](sa_p).squeeze(1))

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        return a, b

    res = {}
    for name, pair in (("grad", (hip_grad, torch_grad)), ("reward", (hip_reward, torch_reward))):
        for _ in range(5):                      # warm both
            for fn in pair:
                fn()
        torch.cuda.synchronize()
        evs = ([], [])
        for _ in range(launches):               # alternate launch by launch
            for k, fn in enumerate(pair):
                evs[k].append(timed(fn))
        torch.cuda.synchronize()
        res[name] = {"hip": _spread([a.elapsed_time(b) for a, b in evs[0]]), "torch": _spread([a.elapsed_time(b) for a, b in evs[1]])}
        res[name]["torch_over_hip"] = res[name]["torch"]["median_ms"] / res[name]["hip"]["median_ms"]
    # the two compute the same thing (f32 tolerance; tests/test_gpu_gail.py holds the f64 parity)
    hip_grad()
    torch_grad()
    ref = torch.cat([p.grad.reshape(-1) for p in net.parameters()])
    res["grad"]["rel_l2_hip_vs_torch"] = float((grad - ref).norm() / ref.norm())
    hip_reward()
    res["reward"]["max_abs_hip_vs_torch"] = float((out - torch_reward()).abs().max())
    res["shape"] = {"policy_rows": n_p, "expert_rows": N_EXPERT, "obs_dim": OD, "n_act": NA, "launches": launches}
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res))


def step_loop(iters):
    import numpy as np
    import torch
    from uavppo.gail import GAILTrainer
    from uavppo.trainer import VecPPOTrainer
    dev = "cuda:0"
    rng = np.random.RandomState(0)
    expert = (rng.rand(N_EXPERT, OD).astype(np.float32), rng.randint(0, NA, N_EXPERT))
    plain = VecPPOTrainer(N_ENV, T, "lstm", hidden=128, device=dev, seed=1)
    gail = GAILTrainer(N_ENV, T, "lstm", hidden=128, device=dev, seed=1, expert=expert)

    def run(tr, k):
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(k):
            tr.train_iteration()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3 / k

    for tr in (plain, gail):
        run(tr, 10)                             # warm-up
    ms = {"plain": [], "gail": []}
    for _ in range(4):                          # A/B/A/B
        ms["plain"].append(run(plain, iters))
        ms["gail"].append(run(gail, iters))
    plain.losses()
    gail.losses()
    el, pl, acc = gail.disc_losses()
    res = {"ms_per_iteration": ms, "plain_median_ms": statistics.median(ms["plain"]), "gail_median_ms": statistics.median(ms["gail"]),
           "iters_per_block": iters, "disc_losses": [el, pl, acc], "shape": {"num_envs": N_ENV, "horizon": T, "policy": "lstm h=128",
                                                                              "expert_rows": N_EXPERT}}
    res["gail_share_of_iteration"] = 1.0 - res["plain_median_ms"] / res["gail_median_ms"]
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=("kernels", "loop"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gail_perf.json"))
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--iters", type=int, default=40)
    a = ap.parse_args()
    if a.step == "kernels":
        return step_kernels(a.launches)
    if a.step == "loop":
        return step_loop(a.iters)
    out = {}
    for step, limit in (("kernels", 240), ("loop", 300)):          # chained: the first failure ends the run
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", step, "--launches", str(a.launches),
               "--iters", str(a.iters)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-4000:] + r.stderr[-4000:])
            raise SystemExit(f"perf_gail: step {step} ended with status {r.returncode}; nothing more is started")
        out[step] = json.loads(r.stdout.strip().splitlines()[-1])
        print(f"[{step}] " + json.dumps(out[step]))
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
