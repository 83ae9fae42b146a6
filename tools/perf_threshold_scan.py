"""The PPOV2.0 threshold stop rule on the device (uav_threshold_windows + one batched predictor call + uav_threshold_rule) against its
host replay: 1000 envs, v2.0, the default ConcentrationThresholdPredictor (hidden 128), the MLP and the h = 128 LSTM policy on the
fused greedy kernels.

    python tools/perf_threshold_scan.py [--out profiles/threshold_scan_perf.json] [--repeats 5] [--launches 40] [--n 1000] [--cap 300]

  (a) evaluate(fused=True, threshold_device=True) against the same call with the default host replay (per env step: roll + column
      write, the rule's dozen small torch launches, the bookkeeping wheres; every 10th step a three-layer LSTM pass over N windows),
      per policy: wall clock between device synchronisations, the sides alternating, median and range of --repeats runs after a
      warm-up round.  The run asserts that both sides return identical metrics.
  (b) one 50-step chunk, HIP events, --launches warm launches, median and range: uav_threshold_windows, the batched predictor call
      over its N * 5 rows, uav_threshold_rule (with the copies that reset its state between launches, which are
      timed alone beside it) -- and one update step's predictor call of the replay (N rows).  The launch counts of either side are
      read from the code and written out beside the times.
The JSON is rewritten after every finished measurement."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "uav-wrf-les-ppo-lstm_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import evaluate_with_lstm as ev  # noqa: E402
from uavppo import ops  # noqa: E402
from uavppo.policy import LSTMActorCritic, MLPActorCritic  # noqa: E402
from uavppo.vec_env import VecMethaneEnv  # noqa: E402

TOWARDS = [0.0, 2.0, -5.0, 2.0, -5.0]        # head bias: +x / +y from the corner, across the field
RULE = dict(window=10, every=10, min_steps=20)


def _stats(ms):
    ms = sorted(ms)
    return {"median_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1], "n": len(ms)}


def _predictor(dev, bias):
    pred = ev.ConcentrationThresholdPredictor(device=dev, seed=4)          # hidden 128, the reference's default
    pred.fc["fc.4.bias"].fill_(bias)             # thresholds inside the plume's concentration range: the rule stops some episodes
    pred.fc["fc.4.weight"].mul_(6.0)
    return pred


def _policy(kind, dev):
    if kind == "mlp":
        pol = MLPActorCritic(6, 5, device=dev, seed=8)
        pol.views["head.weight"][:5].mul_(40.0)
    else:
        pol = LSTMActorCritic(6, 128, 1, device=dev, seed=5)
        pol.views["head.weight"][:5].mul_(400.0)
    pol.views["head.bias"][:5].copy_(torch.tensor(TOWARDS))
    return pol


def evaluation(a, dev, out, save):
    N, cap = a.n, a.cap
    pred = _predictor(dev, a.bias)
    rows = {}
    for kind in ("mlp", "lstm128"):
        pol = _policy(kind, dev)
        env = VecMethaneEnv(N, "v2.0", dev, seed=7)
        sides = {"device": {"threshold_device": True}, "host_replay": {}}
        times, res = {k: [] for k in sides}, {}
        for rep in range(a.repeats + 1):                 # the first round warms every side up
            for name, kw in sides.items():
                ctl = ev.ThresholdController(pred, (0.0, 100.0), N, device=dev)
                torch.cuda.synchronize()
                t = time.perf_counter()
                m = ev.evaluate(pol, env, ctl, max_steps=cap, fused=True, **kw)
                torch.cuda.synchronize()
                if rep:
                    times[name].append((time.perf_counter() - t) * 1e3)
                res[name] = m
        for k in res["device"]:
            assert np.array_equal(res["device"][k], res["host_replay"][k], equal_nan=True), (kind, k)
        st = {k: _stats(v) for k, v in times.items()}
        m = res["device"]
        rows[kind] = dict(st, speedup_of_medians=st["host_replay"]["median_ms"] / st["device"]["median_ms"],
                          device_max_below_replay_min=bool(st["device"]["max_ms"] < st["host_replay"]["min_ms"]),
                          identical_metrics=True, env_steps=int(m["steps"].sum()), mean_steps=float(m["steps"].mean()),
                          stopped_by_rule=float(m["stopped_early"].mean()), ran_to_cap=int((m["steps"] == cap).sum()))
        out["evaluation"] = rows
        save()
        print(json.dumps({"evaluation": {kind: rows[kind]}}), flush=True)


def _timed(fn, launches):
    ms = []
    for i in range(5 + launches):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if i >= 5:
            ms.append(e0.elapsed_time(e1))
    return _stats(ms)


def chunk(a, dev, out, save):
    N, k = a.n, 50
    S = ops.threshold_slots(k, RULE["every"])
    pred = _predictor(dev, a.bias)
    g = torch.Generator().manual_seed(0)
    obs = (torch.rand(N, k, 6, generator=g) * 0.3).to(dev)          # the records' layout: column 2 is read in place
    hist0 = (torch.rand(N, RULE["window"] - 1, generator=g) * 0.3).to(dev)
    series = obs[:, :, 2]
    hist, cnt = hist0.clone(), torch.full((N,), 50, dtype=torch.int32, device=dev)          # an episode's second chunk: 5 update steps
    thr = torch.full((N,), float("nan"), dtype=torch.float64, device=dev)
    x = ops.threshold_windows(series, hist, cnt, lo=0.0, scale=100.0, **RULE)
    rows_in = x.reshape(N * S, RULE["window"], 1)
    p = pred(rows_in).reshape(N, S).contiguous()

    def rule():
        hist.copy_(hist0)
        cnt.fill_(50)
        thr.fill_(float("nan"))
        return ops.threshold_rule(series, hist, cnt, p, thr, want_steps=False, **RULE)

    reset = _timed(lambda: (hist.copy_(hist0), cnt.fill_(50), thr.fill_(float("nan"))), a.launches)
    rows = {"threshold_windows": _timed(lambda: ops.threshold_windows(series, hist, cnt, lo=0.0, scale=100.0, **RULE), a.launches),
            "predictor_batched": dict(_timed(lambda: pred(rows_in), a.launches), rows=N * S, steps=RULE["window"], hidden=128),
            "threshold_rule_with_state_reset": _timed(rule, a.launches), "state_reset_alone": reset,
            "predictor_one_update_step_of_the_replay": dict(_timed(lambda: pred(rows_in[:N]), a.launches), rows=N)}
    first = rule()[0]
    out["chunk"] = dict(rows, shape={"envs": N, "steps": k, "slots": S, "window": RULE["window"]}, envs_with_a_hit=int((first >= 0).sum()),
                        timed="HIP events around each call",
                        device_side_launches_per_chunk="10 calls: uav_threshold_windows, the predictor's zero state fill, 3 uav_lstm_fwd, the "
                        "last-step slice copy, uav_gemm_f32, uav_ln_relu, uav_gemm_f32, uav_threshold_rule; then about a dozen torch "
                        "kernels for the vectorised episode end",
                        replay_side_launches_per_step="push: roll, column write, count += 1; should_stop: about ten small torch kernels; "
                        "bookkeeping: about a dozen where / and / or; every 10th step the predictor over N rows")
    save()
    print(json.dumps({"chunk": out["chunk"]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "threshold_scan_perf.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--launches", type=int, default=40)
    ap.add_argument("--n", type=int, default=1000)
    ap.add_argument("--cap", type=int, default=300)
    ap.add_argument("--bias", type=float, default=18.0, help="fc.4.bias of the threshold predictor (concentration units)")
    a = ap.parse_args()
    dev = "cuda:0"
    out = {"shape": {"envs": a.n, "variant": "v2.0", "cap": a.cap, "predictor": "ConcentrationThresholdPredictor hidden 128",
                     "policies": ["mlp 6-256-128-5", "lstm h=128"], "chunk": 50, "predictor_bias": a.bias},
           "device": torch.cuda.get_device_name(0)}

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")

    chunk(a, dev, out, save)
    evaluation(a, dev, out, save)


if __name__ == "__main__":
    main()
