"""What truncated BPTT does to the time of update() -> profiles/bptt_chunks_perf.json.

VecPPOTrainer(bptt_len=Lc) runs the update's sequence kernels on N * T / Lc sequences of Lc steps instead of N of T: T / Lc
times the workgroups, each with Lc / T of the dependent chain.  This tool measures ms per update() (epochs = 5, one minibatch)
for bptt_len in {T (full BPTT), 32, 16} at

    c2        256 envs x  64 steps, h =  64
    c4       1024 envs x 128 steps, h = 128
    c3_over8  512 envs x 128 steps, h = 128       (C3's envs split over 8 ranks: one rank's share)
    c3       4096 envs x 128 steps, h = 128

All variants of a shape live in ONE process and alternate round by round: every round each variant collects a rollout (not
timed) and then runs update() between two HIP events, as train_iteration() does -- so epoch 0 adopts the rollout's forward
pass in every variant and the chunked ones read their start states out of it.  `--warmup` rounds are discarded, `--rounds`
are kept.  The ratio recorded per chunked variant is its median over the full-BPTT median of the same process.  What chunking
does to LEARNING speed (gradients no longer cross chunk boundaries) is not measured here or anywhere else.

    python tools/perf_bptt_chunks.py [--out profiles/bptt_chunks_perf.json] [--rounds 20] [--warmup 5] [--shapes c2,c4,...]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "uav-wrf-les-ppo-lstm_amd")]

SHAPES = {"c2": dict(N=256, T=64, H=64), "c4": dict(N=1024, T=128, H=128), "c3_over8": dict(N=512, T=128, H=128),
          "c3": dict(N=4096, T=128, H=128)}
CHUNKS = (32, 16)
EPOCHS = 5
DEV = "cuda:0"


def _spread(ms):
    ms = sorted(ms)
    return {"median_ms": statistics.median(ms), "min_ms": ms[0], "max_ms": ms[-1], "p10_ms": ms[len(ms) // 10],
            "p90_ms": ms[(9 * len(ms)) // 10], "n": len(ms)}


def measure(shape, warmup, rounds):
    import torch
    from uavppo.trainer import VecPPOTrainer
    N, T, H = shape["N"], shape["T"], shape["H"]
    variants = {"full": None}
    variants.update({f"bptt_{c}": c for c in CHUNKS if c < T and T % c == 0})
    trainers = {k: VecPPOTrainer(N, T, "lstm", hidden=H, device=DEV, seed=1, use_curriculum=False, epochs=EPOCHS, bptt_len=c)
                for k, c in variants.items()}
    ms = {k: [] for k in trainers}
    for r in range(warmup + rounds):
        for k, tr in trainers.items():
            tr.collect()
            assert tr._rollout_forward_valid            # the fused rollout: epoch 0 adopts its forward pass
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            tr.update()
            b.record()
            b.synchronize()
            if r >= warmup:
                ms[k].append(a.elapsed_time(b))
            tr.iteration += 1
    for tr in trainers.values():
        tr.losses()                                     # raises on NaN
    out = {"shape": dict(shape, epochs=EPOCHS, num_minibatches=1, policy="lstm"), "warmup_rounds": warmup, "rounds": rounds}
    out.update({k: dict(_spread(v), bptt_len=variants[k] or T, sequences=N * T // (variants[k] or T),
                        workgroups_of_16_sequences=-(-(N * T // (variants[k] or T)) // 16)) for k, v in ms.items()})
    for k in trainers:
        if k != "full":
            out[k]["median_over_full"] = out[k]["median_ms"] / out["full"]["median_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bptt_chunks_perf.json"))
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("perf_bptt_chunks.py measures on the GPU: none is visible")
    out = {"what": "ms per update() after a collect(), HIP events, variants alternating in one process; learning speed not measured",
           "device": torch.cuda.get_device_name(0), "compute_units": torch.cuda.get_device_properties(0).multi_processor_count,
           "torch": torch.__version__, "hip": torch.version.hip, "shapes": {}}
    for name in a.shapes.split(","):
        out["shapes"][name] = r = measure(SHAPES[name], a.warmup, a.rounds)
        print(name, {k: (round(v["median_ms"], 3), round(v.get("median_over_full", 1.0), 3)) for k, v in r.items()
                     if isinstance(v, dict) and "median_ms" in v}, file=sys.stderr, flush=True)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
