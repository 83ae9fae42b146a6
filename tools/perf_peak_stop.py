"""The PPOV2.1 peak-and-stop rule on the device (uav_peak_stop_scan) against its host replay: 1000 envs, v2.1, 300-step cap, the
h = 128 LSTM policy on the fused greedy kernels, a PeakAndStopPredictor whose rule stops most but not all episodes.

    python tools/perf_peak_stop.py [--out profiles/peak_stop_perf.json] [--repeats 5] [--launches 40] [--n 1000] [--cap 300]

  (a) evaluate(fused=True, peak_stop_device=True) against the same call with the default host replay (roll + uav_lstm_fwd +
      uav_gemm_f32 + sigmoid per env step), and the device side once more with chunk = 250: wall clock between device
      synchronisations, the sides alternating, median and range of --repeats runs after a warm-up round.  The run asserts that
      all sides return the same `steps` and `stopped_early`.
  (b) one uav_peak_stop_scan (scan kernel + its one-thread-per-env finish kernel) over a 1000 x 50 chunk, HIP events, --launches
      warm launches, median and range -- with full histories (all 50,000 windows valid) and as an episode's first chunk (windows
      from step 20 on).  Beside it the MFMA count of the launch (64 v_mfma_f32_16x16x4_f32 per LSTM step of a 16-window tile
      that holds a valid window) and the time those take at 32 cycles each over the device's SIMDs: the arithmetic floor.
The JSON is rewritten after every finished measurement."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "uav-wrf-les-ppo-lstm_amd")]

import torch  # noqa: E402

import evaluate_with_lstm as ev  # noqa: E402
from uavppo import ops  # noqa: E402
from uavppo.policy import LSTMActorCritic  # noqa: E402
from uavppo.vec_env import VecMethaneEnv  # noqa: E402

TOWARDS = [0.0, 2.0, -5.0, 2.0, -5.0]        # head bias: +x / +y from the corner, across the field
WINDOW = 20


def _stats(ms):
    ms = sorted(ms)
    return {"median_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1], "n": len(ms)}


def _predictor(dev, gain):
    pred = ev.PeakAndStopPredictor(device=dev, seed=10)
    pred.heads_w[1].mul_(12.0)                   # a decisive stop head ...
    pred.lstm.p["weight_ih_l0"].mul_(gain)       # ... on an LSTM that responds to concentrations / 100 of a few hundredths
    return pred


def evaluation(a, dev, out, save):
    N, cap = a.n, a.cap
    pol = LSTMActorCritic(6, 128, 1, device=dev, seed=5)
    pol.views["head.weight"][:5].mul_(400.0)
    pol.views["head.bias"][:5].copy_(torch.tensor(TOWARDS))
    pred = _predictor(dev, a.gain)
    env = VecMethaneEnv(N, "v2.1", dev, seed=7)
    sides = {"device": {"peak_stop_device": True}, "host_replay": {}, "device_chunk250": {"peak_stop_device": True, "chunk": 250}}
    times, res = {k: [] for k in sides}, {}
    for rep in range(a.repeats + 1):                 # the first round warms every side up
        for name, kw in sides.items():
            torch.cuda.synchronize()
            t = time.perf_counter()
            m = ev.evaluate(pol, env, None, peak_stop=pred, max_steps=cap, fused=True, **kw)
            torch.cuda.synchronize()
            if rep:
                times[name].append((time.perf_counter() - t) * 1e3)
            res[name] = m
    for name in ("host_replay", "device_chunk250"):
        for k in ("steps", "stopped_early"):
            assert (res["device"][k] == res[name][k]).all(), (name, k)
    st = {k: _stats(v) for k, v in times.items()}
    m = res["device"]
    row = dict(st, speedup_of_medians=st["host_replay"]["median_ms"] / st["device"]["median_ms"],
               device_max_below_replay_min=bool(st["device"]["max_ms"] < st["host_replay"]["min_ms"]),
               same_steps_and_stops=True, env_steps=int(m["steps"].sum()), mean_steps=float(m["steps"].mean()),
               stopped_by_rule=float(m["stopped_early"].mean()), ran_to_cap=int((m["steps"] == cap).sum()))
    out["evaluation"] = row
    save()
    print(json.dumps({"evaluation": row}), flush=True)


def kernel(a, dev, out, save):
    N, k = a.n, 50
    pred = _predictor(dev, a.gain)
    params = pred.flat_params()
    g = torch.Generator().manual_seed(0)
    obs = (torch.rand(N, k, 6, generator=g) * 0.1).to(dev)          # the records' layout: column 2 is read in place
    hist0 = (torch.rand(N, WINDOW - 1, generator=g) * 0.1).to(dev)
    props = torch.cuda.get_device_properties(0)
    # clock_rate is in kHz; a torch build whose properties lack it: the MI355X's 2.4 GHz peak engine clock
    simds, clock_hz = props.multi_processor_count * 4, getattr(props, "clock_rate", 2.4e6) * 1e3
    rows = {}
    for name, cnt0 in (("full_history", WINDOW - 1), ("first_chunk", 0)):
        hist, cnt = hist0.clone(), torch.full((N,), cnt0, dtype=torch.int32, device=dev)
        ms = []
        for i in range(5 + a.launches):
            hist.copy_(hist0)
            cnt.fill_(cnt0)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            first, _, _ = ops.peak_stop_scan(params, 32, WINDOW, obs[:, :, 2], hist, cnt)
            e1.record()
            e1.synchronize()
            if i >= 5:
                ms.append(e0.elapsed_time(e1))
        valid = (cnt0 + torch.arange(k) + 1 >= WINDOW).repeat(N)               # flattened (env, step) windows
        pad = (-valid.numel()) % 16
        tiles = int(torch.cat([valid, torch.zeros(pad, dtype=torch.bool)]).reshape(-1, 16).any(1).sum())
        mfma = tiles * WINDOW * 64
        rows[name] = dict(_stats(ms), valid_windows=int(valid.sum()), tiles_with_a_valid_window=tiles, mfma_per_launch=mfma,
                          mfma_floor_us=mfma * 32 / simds / clock_hz * 1e6, envs_with_a_hit=int((first >= 0).sum()))
    out["scan_launch"] = dict(rows, shape={"envs": N, "steps": k, "window": WINDOW}, simds=simds, clock_mhz=clock_hz / 1e6,
                              timed="scan kernel + finish kernel, HIP events")
    save()
    print(json.dumps({"scan_launch": out["scan_launch"]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "peak_stop_perf.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--launches", type=int, default=40)
    ap.add_argument("--n", type=int, default=1000)
    ap.add_argument("--cap", type=int, default=300)
    ap.add_argument("--gain", type=float, default=250.0, help="input gain of the stop predictor's LSTM")
    a = ap.parse_args()
    dev = "cuda:0"
    out = {"shape": {"envs": a.n, "variant": "v2.1", "cap": a.cap, "policy": "lstm h=128", "window": WINDOW, "input_gain": a.gain},
           "device": torch.cuda.get_device_name(0)}

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")

    kernel(a, dev, out, save)
    evaluation(a, dev, out, save)


if __name__ == "__main__":
    main()
