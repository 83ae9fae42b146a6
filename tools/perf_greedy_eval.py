"""Greedy evaluation throughput: evaluate_with_lstm.evaluate on the fused greedy-episode kernels (uav_greedy_episodes) against
its step-wise path, for the LSTM actor-critic (h = 128) and the reference's MLP, N in {1000, 4096}, 1000-step cap, without and
with the PPOV2.0 stop controller.  Fused and step-wise alternate, 3 repeats each after a warm-up; wall clock between device
synchronisations.  One JSON line per case.  Kernel times: run it under `rocprofv3 --kernel-trace --stats -- python ...`.

    python tools/perf_greedy_eval.py [--n 1000 4096] [--repeats 3] [--cap 1000]
    python tools/perf_greedy_eval.py --eval-v11 OUT.json [--parent-lib PATH] [--repeats 3] [--blocks 4] [--per-block 5]
    python tools/perf_greedy_eval.py --chunk mlp|lstm128

--eval-v11 OUT.json measures evaluate_model.ModelEvaluator instead (1000 envs, v1.1, 2000-step cap, the reference's MLP and
the h = 128 LSTM, bias-forced policies that cross the field before they settle):
  (a) run_evaluation on the fused kernels (the stop rule on the device) against the same evaluation step-wise (fused=False:
      the rule through uav_stop_stability once per step); wall clock between device synchronisations (the host's record
      reduction is part of what is measured), alternating, median and range of --repeats runs after a warm-up round;
  (b) one chunk of uav_greedy_episodes_stop under a rule that cannot fire against uav_greedy_episodes at the same shape and
      chunk, every launch from the same reset state: warm launches, HIP events, median and range, A and B alternating in
      blocks.  With --parent-lib PATH a child process (--chunk KIND under UAVPPO_LIB=PATH) times uav_greedy_episodes of that
      library build the same way.
OUT.json is rewritten after every finished measurement, so a run that ends early leaves what it had measured.
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


TOWARDS = [0.0, 2.0, -5.0, 2.0, -5.0]        # head bias: +x / +y from the corner, across the field


def _v11_policy(kind, dev):
    if kind == "mlp":
        pol = MLPActorCritic(6, 5, device=dev, seed=3)
        pol.views["head.weight"][:5].mul_(40.0)
    else:
        pol = LSTMActorCritic(6, 128, 1, device=dev, seed=5)
        pol.views["head.weight"][:5].mul_(400.0)
    pol.views["head.bias"][:5].copy_(torch.tensor(TOWARDS))
    return pol


def _stats(ms):
    ms = sorted(ms)
    return {"median_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1], "n": len(ms)}


def _chunk_times(kind, N, chunk, dev, blocks, per_block, with_stop=True):
    """HIP-event times of one `chunk`-step launch from the reset state: uav_greedy_episodes (A) and uav_greedy_episodes_stop
    under a rule that cannot fire (B), alternating in blocks of `per_block` launches after warm launches of both; A alone
    with with_stop=False."""
    from uavppo import ops
    pol = _v11_policy(kind, dev)
    H = 0 if kind == "mlp" else 128
    env = VecMethaneEnv(N, "v1.1", dev, seed=7)
    h = torch.zeros(N, H, device=dev) if H else None
    c = torch.zeros(N, H, device=dev) if H else None
    active = torch.ones(N, dtype=torch.uint8, device=dev)
    recs = ops.greedy_recs(N, chunk, 6, dev)
    never = ops.make_stop_rule(pos_std_max=0.0) if with_stop else None
    win = torch.zeros(N, 10, 2, device=dev)
    cnt = torch.zeros(N, dtype=torch.int32, device=dev)

    def launch(stop):
        env.reset()
        active.fill_(1)
        cnt.zero_()
        if H:
            h.zero_()
            c.zero_()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        if stop:
            ops.greedy_episodes_stop(env.state, N, env.cfg(), pol.flat, H, chunk, env.obs, h, c, active, recs, never, win, cnt)
        else:
            ops.greedy_episodes(env.state, N, env.cfg(), pol.flat, H, chunk, env.obs, h, c, active, recs)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), int(((recs["flags"] & 4) == 0).sum())

    kinds = (False, True) if with_stop else (False,)
    for stop in kinds:
        for _ in range(3):
            launch(stop)
    times, env_steps = {k: [] for k in kinds}, {}
    for _ in range(blocks):
        for stop in kinds:
            for _ in range(per_block):
                ms, n = launch(stop)
                times[stop].append(ms)
                env_steps[stop] = n
    return {("stop_never_fires" if k else "plain"): dict(_stats(v), env_steps=env_steps[k]) for k, v in times.items()}


def _bind_library():
    """Load the library UAVPPO_LIB names (or the tree's) and bind the entry points it has, so that a build from before
    uav_greedy_episodes_stop existed can be timed too: calling one it lacks raises AttributeError.  -> has the stop entry."""
    import ctypes
    from uavppo import _lib
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name, (res, args) in _lib.SIGNATURES.items():
        fn = getattr(handle, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = res, args
    _lib._lib = handle
    return hasattr(handle, "uav_greedy_episodes_stop")


def _chunk_row(kind, N, blocks, per_block):
    ch = _chunk_times(kind, N, 250, "cuda:0", blocks, per_block, with_stop=_bind_library())
    if "stop_never_fires" in ch:
        ch["stop_over_plain_medians"] = ch["stop_never_fires"]["median_ms"] / ch["plain"]["median_ms"]
    return ch


def eval_v11(a):
    import subprocess
    import evaluate_model as em
    dev = "cuda:0"
    N, cap, chunk = a.n[0], a.cap, 250
    out = {"shape": {"envs": N, "variant": "v1.1", "cap": cap, "chunk": chunk}, "device": torch.cuda.get_device_name(0),
           "evaluation": {}, "chunk_launch": {}}

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(a.eval_v11)), exist_ok=True)
        with open(a.eval_v11, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")

    for kind in ("mlp", "lstm128"):
        ch = _chunk_row(kind, N, a.blocks, a.per_block)
        if a.parent_lib:
            env = dict(os.environ, UAVPPO_LIB=os.path.abspath(a.parent_lib))
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--chunk", kind, "--n", str(N), "--blocks", str(a.blocks),
                                "--per-block", str(a.per_block)], env=env, capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                raise RuntimeError(f"parent-library child failed ({r.returncode}): {r.stderr[-400:]}")
            ch["plain_parent_library"] = json.loads(r.stdout.strip().splitlines()[-1])["plain"]
        out["chunk_launch"][kind] = ch
        save()
        print(json.dumps({"chunk_launch": kind, **ch}), flush=True)
    for kind in ("mlp", "lstm128"):
        pol = _v11_policy(kind, dev)
        evl = em.ModelEvaluator(pol, eval_episodes=N, device=dev, env=VecMethaneEnv(N, "v1.1", dev, seed=7))
        times, res = {True: [], False: []}, {}
        for rep in range(a.repeats + 1):                        # the first round warms both paths up
            for fused in (True, False):
                torch.cuda.synchronize()
                t = time.perf_counter()
                m = evl.run_evaluation(max_steps=cap, fused=fused, csv_path=None)
                torch.cuda.synchronize()
                if rep:
                    times[fused].append((time.perf_counter() - t) * 1e3)
                res[fused] = m
        same = all((res[True][k] == res[False][k]).all() for k in ("steps", "stopped_early", "success"))
        row = {"fused": _stats(times[True]), "stepwise": _stats(times[False]),
               "speedup_of_medians": _stats(times[False])["median_ms"] / _stats(times[True])["median_ms"],
               "same_steps_stops_success": bool(same), "env_steps": int(res[True]["steps"].sum()),
               "mean_steps": float(res[True]["steps"].mean()), "stopped_by_rule": float(res[True]["stopped_early"].mean()),
               "ran_to_cap": int((res[True]["steps"] == cap).sum()), "stopped_at_step_10": int((res[True]["steps"] == 10).sum())}
        out["evaluation"][kind] = row
        save()
        print(json.dumps({"evaluation": kind, **row}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=None)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--cap", type=int, default=None)
    ap.add_argument("--eval-v11", metavar="OUT.json", default=None)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--chunk", choices=("mlp", "lstm128"), default=None,
                    help="measurement (b) alone for one policy, on the library UAVPPO_LIB names; one JSON line")
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--per-block", type=int, default=5)
    a = ap.parse_args()
    if a.chunk:
        print(json.dumps(_chunk_row(a.chunk, (a.n or [1000])[0], a.blocks, a.per_block)))
        return
    if a.eval_v11:
        a.n, a.cap = a.n or [1000], a.cap or 2000
        return eval_v11(a)
    a.n, a.cap = a.n or [1000, 4096], a.cap or 1000
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
