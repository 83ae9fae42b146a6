"""What the anisotropic-plume kernels cost -> profiles/source_aniso_perf.json.

    kernels    us per call of uav_source_moments6 / uav_source_solve6 / uav_source_summary6 beside uav_source_moments /
               uav_source_solve / uav_source_summary on the same 1024 x 250 x 6 chunk of records (tools/perf_source_fit.py's), each
               between two HIP events, in this one process.
    bank       ms for uav_plume_bank of 64 fields against 64 uav_env_materialise calls (field_bank.synthesise's loop).
    run        one EvalTracker.run() (1024 evaluation envs x 1000 steps, LSTM h = 128, an "aniso:8" bank) with source_fit off, model
               "iso" and model "aniso".

    python tools/perf_source_aniso.py [--what kernels,bank,run] [--out profiles/source_aniso_perf.json] [--rounds 20] [--warmup 5]

HIP events cost several microseconds themselves and a launch about 20: the kernel figures are upper bounds on the kernels' own time.
The registers of the new kernels are the compiler's (-Rpass-analysis=kernel-resource-usage on csrc/source_aniso.hip) and are
recorded by hand under "resources".
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "uav-wrf-les-ppo-lstm_amd"))
DEV = "cuda:0"
N = 1024
# gfx950, hipcc -O3 -ffp-contract=off, the build's flags
RESOURCES = {"plume_bank_kernel": {"vgprs": 38, "spills": 0, "scratch": 0, "waves_per_simd": 8},
             "source_moments6_kernel": {"vgprs": 172, "spills": 0, "scratch": 0, "waves_per_simd": 2},
             "source_solve6_kernel": {"vgprs": 96, "spills": 0, "scratch": 0, "waves_per_simd": 5},
             "source_summary6_kernel": {"vgprs": 76, "spills": 0, "scratch": 0, "lds_bytes": 32, "waves_per_simd": 6}}


def _time(torch, fn, warmup, rounds):
    """median / min / max microseconds of fn() between two HIP events"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        us.append(a.elapsed_time(b) * 1000.0)
    return {"median_us": statistics.median(us), "min_us": min(us), "max_us": max(us)}


def kernels(torch, warmup, rounds):
    import perf_source_fit as psf
    from uavppo import ops
    recs, src = psf._records(torch)
    c4, c6 = ops.source_fit_cfg(), ops.source_fit_cfg(min_samples=8)
    st4 = torch.zeros(N, ops.SRC_STATE_N, dtype=torch.float64, device=DEV)
    st6 = torch.zeros(N, ops.SRC6_STATE_N, dtype=torch.float64, device=DEV)
    est4 = torch.zeros(N, ops.SRC_EST_N, dtype=torch.float64, device=DEV)
    est6 = torch.zeros(N, ops.SRC6_EST_N, dtype=torch.float64, device=DEV)
    status = torch.zeros(N, dtype=torch.uint8, device=DEV)
    s4 = torch.zeros(ops.SRC_SUM_N, dtype=torch.float64, device=DEV)
    s6 = torch.zeros(ops.SRC6_SUM_N, dtype=torch.float64, device=DEV)
    truth = torch.tensor([31.25, 31.25, 0.0, 100.0], dtype=torch.float64, device=DEV).repeat(N, 1).contiguous()

    def fresh(st, fn):
        def go():
            st.zero_()
            fn()
        return go
    out = {"shape": [N, psf.K, psf.D]}
    zero = _time(torch, st6.zero_, warmup, rounds)
    out["state_zero_launch_alone"] = zero
    out["uav_source_moments"] = _time(torch, fresh(st4, lambda: ops.source_moments(recs, c4, st4)), warmup, rounds)
    out["uav_source_moments6"] = _time(torch, fresh(st6, lambda: ops.source_moments6(recs, c6, st6)), warmup, rounds)
    st4.zero_()
    st6.zero_()
    ops.source_moments(recs, c4, st4)
    ops.source_moments6(recs, c6, st6)
    out["uav_source_solve"] = _time(torch, lambda: ops.source_solve(st4, c4, est4, status), warmup, rounds)
    out["uav_source_solve6"] = _time(torch, lambda: ops.source_solve6(st6, c6, est6, status), warmup, rounds)
    out["uav_source_summary"] = _time(torch, lambda: ops.source_summary(est4, status, src, 31.25, 100.0, 5.0, s4), warmup, rounds)
    ops.source_solve6(st6, c6, est6, status)
    out["uav_source_summary6"] = _time(torch, lambda: ops.source_summary6(est6, status, src, truth, 5.0, s6), warmup, rounds)
    out["fitted_of_1024"] = {"six_term": int(s6[1].item()), "four_term": int(s4[1].item())}
    out["note"] = "the two moments figures include one zeroing launch of the state (state_zero_launch_alone)"
    return out


def bank(torch, warmup, rounds):
    import numpy as np
    from uavppo import ops, source_aniso as sa
    from uavppo.vec_env import VecMethaneEnv
    F = 64
    rng = np.random.default_rng(1)
    params = sa.plume_params(rng.uniform(50.0, 450.0, (F, 2)), rng.uniform(20.0, 45.0, F), rng.uniform(8.0, 20.0, F),
                             rng.uniform(0.0, np.pi, F), 100.0)
    out_bank = torch.empty(F, 500, 500, 2, dtype=torch.float64, device=DEV)
    gen = VecMethaneEnv(F, "v2.0", DEV, seed=4321)
    gen.reset()
    cfg = gen.cfg()
    w, r = max(1, warmup // 2), max(3, rounds // 4)
    a = _time(torch, lambda: ops.plume_bank(params, 4321, 0, out=out_bank), w, r)
    b = _time(torch, lambda: [ops.env_materialise(gen.state, F, cfg, f, out=out_bank[f]) for f in range(F)], w, r)
    gb = F * 500 * 500 * 2 * 8 / 1e9
    return {"fields": F, "uav_plume_bank": a, "uav_env_materialise_x64": b, "bytes_written_gb": gb,
            "uav_plume_bank_gb_per_s": gb / (a["median_us"] * 1e-6)}


def run(torch, warmup, rounds):
    from uavppo import field_bank as fb
    from uavppo.eval_track import EvalTracker
    from uavppo.policy import LSTMActorCritic
    b, s, t = fb.load_with_truth("aniso:8", device=DEV)
    out = {"envs": N, "steps": 1000, "policy": "lstm h=128, fresh", "bank": "aniso:8"}
    for name, kw in (("off", {}), ("iso", {"source_fit": True}), ("aniso", {"source_fit": {"model": "aniso"}, "bank_truth": t})):
        pol = LSTMActorCritic(6, 128, 1, device=DEV, seed=3)
        tr = EvalTracker(pol, "lstm", N, "v2.0", bank=b, bank_sources=s, device=DEV, max_steps=1000, **kw)
        it = [0]

        def go():
            it[0] += 1
            tr.run(it[0])
        res = _time(torch, go, max(1, warmup // 2), max(3, rounds // 2))
        rows = tr.curve(wait=True)
        if "source" in rows[-1]:
            res["fitted_of_1024"] = int(rows[-1]["source"][1])
        out[name] = res
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="kernels,bank,run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "source_aniso_perf.json"))
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    import torch
    res = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "warmup": a.warmup, "resources": RESOURCES}
    for what in a.what.split(","):
        res[what] = {"kernels": kernels, "bank": bank, "run": run}[what](torch, a.warmup, a.rounds)
        print(what, json.dumps(res[what]), flush=True)
    res["not_measured"] = ("train_iteration() at C2 / C3 against a build of the parent commit and the kernel-name table of ten C2 "
                           "iterations: with the option off no launch is added (the trainer's iteration code is unchanged)")
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
