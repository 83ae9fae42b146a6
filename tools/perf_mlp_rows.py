"""What a shuffled-row minibatch costs on the fused MLP gradient kernel -> profiles/mlp_rows_perf.json.

Shape: 4096 envs x 128 steps of the reference's MLP (6-256-128, 5 actions) on buffers a rollout filled; one epoch = 8 chunks
of 65,536 rows under one random permutation of the 524,288 rows.

  (a) rows      uav_mlp_ppo_grad_rows on a chunk of the permutation: the kernel gathers its samples through the index;
  (b) gather    what the same optimiser step takes without that entry: six index_select calls (obs, act, logp, adv, ret, val)
                into contiguous buffers allocated once, then uav_mlp_ppo_grad on the copies -- the same gradient, bit for bit
                (asserted here on the first chunk);
  (c) contiguous  uav_mlp_ppo_grad alone on 65,536 contiguous rows: what the gather itself costs is (a) / (c).

HIP events around one chunk's work, the three forms alternating chunk by chunk (every chunk of the permutation is visited by
all three before the next), `--launches` timed launches each after as many warm ones; medians with min / max / p10 / p90.
Acceptance: (a) <= (b) on the medians -- (b) makes strictly more memory passes over the same rows.  (a) / (c) is reported, not
bounded.

    python tools/perf_mlp_rows.py [--out profiles/mlp_rows_perf.json] [--launches 30]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "uav-wrf-les-ppo-lstm_amd")]

N_ENV, T, CHUNK = 4096, 128, 65536
DEV = "cuda:0"


def _spread(ms):
    ms = sorted(ms)
    return {"median_ms": statistics.median(ms), "min_ms": ms[0], "max_ms": ms[-1], "p10_ms": ms[len(ms) // 10],
            "p90_ms": ms[(9 * len(ms)) // 10], "n": len(ms)}


def _event_ms(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mlp_rows_perf.json"))
    ap.add_argument("--launches", type=int, default=30)
    a = ap.parse_args()
    import torch
    from uavppo import ops
    from uavppo.trainer import VecPPOTrainer
    tr = VecPPOTrainer(N_ENV, T, "mlp", device=DEV, seed=1, use_curriculum=False, update_form="inline_v10")
    tr.collect()
    tr.check_ranges()
    tr.compute_advantages()
    L = N_ENV * T
    bufs = [tr.buf["obs"].view(L, 6)] + [x.view(L) for x in (tr.buf["act"], tr.buf["logp"], tr.adv_n, tr.ret, tr.buf["val"])]
    perm = torch.randperm(L, generator=torch.Generator(device=DEV).manual_seed(1), device=DEV)
    chunks32 = [c.contiguous() for c in perm.to(torch.int32).split(CHUNK)]
    chunks64 = [c.contiguous() for c in perm.split(CHUNK)]
    copies = [torch.empty((CHUNK,) + tuple(b.shape[1:]), dtype=b.dtype, device=DEV) for b in bufs]
    head = [b[:CHUNK] for b in bufs]
    sums, inv_n = tr.loss_sums, 1.0 / CHUNK
    grads = {k: torch.empty_like(tr.policy.flat) for k in ("rows", "gather", "contiguous")}

    def rows(i):
        ops.mlp_ppo_grad_rows(tr.policy.flat, *bufs, chunks32[i], inv_n, 0.2, 0.01, sums, grads["rows"])

    def gather(i):
        for src, dst in zip(bufs, copies):
            torch.index_select(src, 0, chunks64[i], out=dst)
        ops.mlp_ppo_grad(tr.policy.flat, *copies, inv_n, 0.2, 0.01, sums, grads["gather"])

    def contiguous(i):
        ops.mlp_ppo_grad(tr.policy.flat, *head, inv_n, 0.2, 0.01, sums, grads["contiguous"])

    fns = {"rows": rows, "gather": gather, "contiguous": contiguous}
    rows(0)
    gather(0)
    torch.cuda.synchronize()
    same = bool(torch.equal(grads["rows"], grads["gather"]))
    ms = {k: [] for k in fns}
    for timed in (False, True):                  # as many warm launches as timed ones, in the same order
        for n in range(a.launches):
            for k, fn in fns.items():
                t = _event_ms(lambda: fn(n % len(chunks32)))
                if timed:
                    ms[k].append(t)
    out = {"shape": {"envs": N_ENV, "T": T, "rows": L, "chunk_rows": CHUNK, "chunks_per_epoch": L // CHUNK, "policy": "mlp 6-256-128",
                     "arith": tr.arith},
           "launches": a.launches, "device": torch.cuda.get_device_name(0), "rows_equals_gather_bitwise": same}
    out.update({k: _spread(v) for k, v in ms.items()})
    out["epoch_ms"] = {k: out[k]["median_ms"] * (L // CHUNK) for k in fns}
    out["rows_over_gather_medians"] = out["rows"]["median_ms"] / out["gather"]["median_ms"]
    out["rows_over_contiguous_medians"] = out["rows"]["median_ms"] / out["contiguous"]["median_ms"]
    out["accepted_rows_le_gather"] = out["rows"]["median_ms"] <= out["gather"]["median_ms"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)
    if not (same and out["accepted_rows_le_gather"]):
        raise SystemExit("acceptance failed: rows must equal gather bit for bit and be no slower")


if __name__ == "__main__":
    main()
