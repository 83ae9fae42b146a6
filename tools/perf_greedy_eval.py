"""Greedy evaluation throughput: evaluate_with_lstm.evaluate on the fused greedy-episode kernels (uav_greedy_episodes) against
its step-wise path, for the LSTM actor-critic (h = 128) and the reference's MLP, N in {1000, 4096}, 1000-step cap, without and
with the PPOV2.0 stop controller.  Fused and step-wise alternate, 3 repeats each after a warm-up; wall clock between device
synchronisations.  One JSON line per case.  Kernel times: run it under `rocprofv3 --kernel-trace --stats -- python ...`.

    python tools/perf_greedy_eval.py [--n 1000 4096] [--repeats 3] [--cap 1000]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "uav-wrf-les-ppo-lstm_amd")]

import torch  # noqa: E402

import evaluate_with_lstm as ev  # noqa: E402
from uavppo.policy import LSTMActorCritic, MLPActorCritic  # noqa: E402
from uavppo.vec_env import VecMethaneEnv  # noqa: E402


def _run(pol, env, ctl, fused, cap):
    torch.cuda.synchronize()
    t = time.perf_counter()
    m = ev.evaluate(pol, env, ctl, max_steps=cap, fused=fused)
    torch.cuda.synchronize()
    return time.perf_counter() - t, m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[1000, 4096])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--cap", type=int, default=1000)
    a = ap.parse_args()
    dev = "cuda:0"
    for kind in ("lstm128", "mlp"):
        for N in a.n:
            pol = LSTMActorCritic(6, 128, 1, device=dev, seed=1) if kind == "lstm128" else MLPActorCritic(6, 5, device=dev, seed=1)
            for controller in (False, True):
                env = VecMethaneEnv(N, "v2.0", dev, seed=7)
                ctl = ev.ThresholdController(ev.ConcentrationThresholdPredictor(device=dev, seed=2), (0.0, 100.0), N, device=dev) \
                    if controller else None
                times = {True: [], False: []}
                steps = {}
                for fused in (True, False):                     # warm-up
                    _run(pol, env, ctl, fused, a.cap)
                for _ in range(a.repeats):
                    for fused in (True, False):
                        dt, m = _run(pol, env, ctl, fused, a.cap)
                        times[fused].append(dt)
                        steps[fused] = int(m["steps"].sum())
                row = {"policy": kind, "N": N, "cap": a.cap, "controller": "v2.0" if controller else None}
                for fused, name in ((True, "fused"), (False, "stepwise")):
                    best = min(times[fused])
                    row[name] = {"s": times[fused], "episodes_per_s": N / best, "env_steps_per_s": steps[fused] / best,
                                 "env_steps": steps[fused]}
                row["speedup"] = min(times[False]) / min(times[True])
                print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
