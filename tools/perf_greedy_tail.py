"""Greedy evaluation on the tail route (the LSTM layers' step kernels + one uav_greedy_tail per env step, uavppo.greedy.GreedyRun
(tail=True)) against the step-wise loop the same call takes with tail=False: 1000 envs, v2.1, 300-step cap.

    python tools/perf_greedy_tail.py [--out profiles/greedy_tail_perf.json] [--repeats 5] [--n 1000] [--cap 300]

  (a) the C5 policy, h = 256 x 2 with trend_k = 2 (layers on ops.LstmStepper: 4 launches per env step), evaluate();
  (b) h = 128 x 2 (layers on uav_lstm_fwd with T = 1: 7 launches per env step), evaluate();
  (c) the policy of (a) at trend_k = 0 on a v1.1 env through ModelEvaluator.run_evaluation with its stop rule.
Both sides of a configuration run in one process, alternating; wall clock between device synchronisations; median and range of
--repeats runs after a warm-up round; the run asserts that both sides return identical arrays before any time is kept.  Without
--config the script runs the three configurations as child processes, each under its own `timeout`, and stops at the first that
fails; each child adds its row to the JSON."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "uav-wrf-les-ppo-lstm_amd")]
LSTM_GAIN = 8.0                              # on the LSTM weights: greedy actions that depend on the observation and on (h, c)
CONFIGS = {"a": "C5: LSTM h=256 x 2, trend_k=2, evaluate()", "b": "LSTM h=128 x 2 (per-call layers), evaluate()",
           "c": "LSTM h=256 x 2, ModelEvaluator.run_evaluation with its stop rule (v1.1 env)"}


def _stats(ms):
    ms = sorted(ms)
    return {"median_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1], "n": len(ms)}


def _policy(H, obs_dim, dev):
    import torch
    from uavppo.policy import LSTMActorCritic
    pol = LSTMActorCritic(obs_dim, H, 2, device=dev, seed=5)
    for k, v in pol.views.items():
        if k.startswith("lstm.weight"):
            v.mul_(LSTM_GAIN)
    pol.views["head.weight"][:5].mul_(400.0)
    return pol


def one_config(a):
    import numpy as np
    import torch
    import evaluate_model as em
    import evaluate_with_lstm as ev
    from uavppo.vec_env import VecMethaneEnv
    dev, N, cap = "cuda:0", a.n, a.cap
    if a.config == "c":
        pol = _policy(256, 6, dev)
        evl = em.ModelEvaluator(pol, eval_episodes=N, device=dev, env=VecMethaneEnv(N, "v1.1", dev, seed=7))
        run = lambda **kw: evl.run_evaluation(max_steps=cap, csv_path=None, **kw)
    else:
        pol = _policy(256, 8, dev) if a.config == "a" else _policy(128, 6, dev)
        env = VecMethaneEnv(N, "v2.1", dev, seed=7, trend_k=pol.obs_dim - 6)
        run = lambda **kw: ev.evaluate(pol, env, max_steps=cap, **kw)
    from uavppo.greedy import GreedyRun
    probe_env = VecMethaneEnv(N, "v1.1" if a.config == "c" else "v2.1", dev, seed=7, trend_k=pol.obs_dim - 6)
    probe_env.reset()
    acts = GreedyRun("lstm", pol, probe_env, tail=True).chunk(0, 50, None)["act"]
    action_counts = torch.bincount(acts[acts >= 0].long(), minlength=5).tolist()       # of the first 50 steps
    assert sum(c > 0 for c in action_counts) >= 3, action_counts
    sides = {"tail": {"tail": True}, "stepwise": {"fused": False, "tail": False}}
    times, res = {k: [] for k in sides}, {}
    for rep in range(a.repeats + 1):                 # the first round warms both sides up and checks identity
        for name, kw in sides.items():
            torch.cuda.synchronize()
            t = time.perf_counter()
            m = run(**kw)
            torch.cuda.synchronize()
            if rep:
                times[name].append((time.perf_counter() - t) * 1e3)
            res[name] = m
        if not rep:
            assert sorted(res["tail"]) == sorted(res["stepwise"])
            for k in res["tail"]:
                assert np.array_equal(res["tail"][k], res["stepwise"][k], equal_nan=True), k
    st = {k: _stats(v) for k, v in times.items()}
    m = res["tail"]
    row = dict(st, what=CONFIGS[a.config], speedup_of_medians=st["stepwise"]["median_ms"] / st["tail"]["median_ms"],
               tail_max_below_stepwise_min=bool(st["tail"]["max_ms"] < st["stepwise"]["min_ms"]), identical_arrays=True,
               launches_per_env_step_tail=4 if a.config != "b" else 7, action_counts_first_50_steps=action_counts, mean_steps=float(m["steps"].mean()),
               ran_to_cap=int((m["steps"] == cap).sum()), stopped_by_rule=float(m["stopped_early"].mean()))
    out = json.load(open(a.out)) if os.path.exists(a.out) else {}
    out.update(shape={"envs": N, "variant": "v2.1 (c: v1.1)", "cap": cap}, device=torch.cuda.get_device_name(0))
    out[a.config] = row
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({a.config: row}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "greedy_tail_perf.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--n", type=int, default=1000)
    ap.add_argument("--cap", type=int, default=300)
    ap.add_argument("--config", choices=sorted(CONFIGS), help="run one configuration in this process")
    ap.add_argument("--limit", type=int, default=300, help="seconds each configuration's child process may take")
    a = ap.parse_args()
    if a.config:
        return one_config(a)
    if os.path.exists(a.out):
        os.remove(a.out)
    for c in sorted(CONFIGS):
        rc = subprocess.run(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--config", c,
                             "--out", a.out, "--repeats", str(a.repeats), "--n", str(a.n), "--cap", str(a.cap)]).returncode
        if rc != 0:
            sys.exit(f"configuration {c} ended with status {rc}: the configurations after it are not run")


if __name__ == "__main__":
    main()
