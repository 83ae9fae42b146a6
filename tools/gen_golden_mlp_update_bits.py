"""Record tests/golden/mlp_update_bits.json: SHA-256 digests of what mlp_ppo_grad_kernel (csrc/mlp_update.hip) writes.

The fused MLP update is the kernel tuned hardest for registers; the tolerance tests against autograd (tests/test_gpu_trainer.py,
test_gpu_trend_mlp.py, test_gpu_inline_update.py, test_gpu_ppo_diag.py) hold it to an oracle but cannot tell "still the same
arithmetic" from "close enough".  tests/test_gpu_mlp_update_bits.py compares the gradient, the loss sums and the diagnostic sums
of the cases below with the digests recorded here -- by the build BEFORE a change to the kernel's source, on the GPU:

    python tools/gen_golden_mlp_update_bits.py [OUT]    # at the parent commit of the change; OUT defaults to the golden file

Inputs come from numpy's RandomState; nothing outside the repository is read.  Parameters stay far below the fp16-split form's
guard (max |param| < 2048).  One gradient slab per workgroup and one workgroup per CU: the summation order depends on the CU
count, which is stored with the digests.

A case is one (sample layout, arithmetic, trend_k): all 16 instantiations (fp16x3 / f32_mfma  x  6 inputs / run-time width  x
contiguous / rows  x  diagnostics off / on) are reached, the run-time width with 7 and with 8 inputs (8 leave no spare column of
X for db1).  A tile is 32 samples; each case runs
    n = 1               one tile with 31 dead sample lanes: the ones column / sample-valid predicate of db1, zeroed X rows
    n = 32, n = 33      an exactly full tile; a second workgroup with one live sample
    n = 2 * 32 * CUs + 7   every workgroup walks two tiles and one a third, partial one: the LDS accumulators carried across
                        tiles, the rows form's prefetch of the next tile's indices and the fp16-split form's running scale --
                        twice: with the advantages of the second half of the samples (= every workgroup's second tile) x 64,
                        so the later tile brings the larger |dz2| and the dW2 accumulators are rescaled, and / 64, so they are not
The rows form draws its indices from 20000-row buffers in random order with repeats (the launch's first half from the buffers'
lower half, its second from the upper), a few of them below 0 and a few >= 20000 (the kernel clamps them: pinned here).
n = 33 and the x 64 run are repeated with the diagnostics attached.
"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "uav-wrf-les-ppo-lstm_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

DEV = "cuda:0"
PATH = os.path.join(ROOT, "tests", "golden", "mlp_update_bits.json")
TILE = 32
N_TOTAL = 20000         # buffer rows of the rows form
CLIP, BETA = 0.2, 0.01
# (tag, n or None = 2 * TILE * CUs + 7, factor on the advantages of the second half, diagnostics attached)
RUNS = (("n1", 1, 1.0, False), ("n32", 32, 1.0, False), ("n33", 33, 1.0, False), ("n33-diag", 33, 1.0, True),
        ("up", None, 64.0, False), ("up-diag", None, 64.0, True), ("down", None, 1.0 / 64.0, False))


def cu_count():
    return int(torch.cuda.get_device_properties(DEV).multi_processor_count)


def _sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _uni(rs, shape, bound):
    return rs.uniform(-bound, bound, size=shape).astype(np.float32)


def mlp_params(rs, D):
    """W1[256][D] b1 g1 be1 W2[128][256] b2 g2 be2 Wh[6][128] bh (csrc/mlp.hip's flat layout); max |param| < 2"""
    parts = [_uni(rs, (256, D), 1.0 / np.sqrt(D)), _uni(rs, 256, 0.1), 1.0 + _uni(rs, 256, 0.1), _uni(rs, 256, 0.1),
             _uni(rs, (128, 256), 1.0 / 16.0), _uni(rs, 128, 0.1), 1.0 + _uni(rs, 128, 0.1), _uni(rs, 128, 0.1),
             _uni(rs, (6, 128), 0.4), _uni(rs, 6, 0.5)]
    return np.concatenate([p.reshape(-1) for p in parts])


def samples(rs, n, D, factor):
    """obs and the five per-sample scalars of n samples; the advantages of samples n // 2 .. are multiplied by `factor`"""
    adv = rs.randn(n).astype(np.float32)
    adv[n // 2:] *= np.float32(factor)
    return {"obs": _uni(rs, (n, D), 2.0), "act": rs.randint(0, 5, size=n).astype(np.int32),
            "logp_old": (-1.6 + 0.3 * rs.randn(n)).astype(np.float32), "adv": adv, "ret": rs.randn(n).astype(np.float32),
            "val_old": (0.5 * rs.randn(n)).astype(np.float32)}


def row_indices(rs, n):
    """n indices into the N_TOTAL-row buffers, random order with repeats: the first half of the launch reads the lower half of
    the buffers, the second half the upper half (so the factor on the advantages follows the launch's order); from n = 32 on,
    four indices of the first half lie below 0 and four of the second past the end"""
    h = n // 2
    rows = np.concatenate([rs.randint(0, N_TOTAL // 2, size=h), rs.randint(N_TOTAL // 2, N_TOTAL, size=n - h)]).astype(np.int32)
    if n >= TILE:
        rows[rs.choice(h, size=4, replace=False)] = np.array([-1, -3, -N_TOTAL, -2 ** 31], dtype=np.int64).astype(np.int32)
        rows[h + rs.choice(n - h, size=4, replace=False)] = np.array([N_TOTAL, N_TOTAL + 5, 2 * N_TOTAL, 2 ** 31 - 1], dtype=np.int64).astype(np.int32)
    return rows


def run_one(layout, k, n, factor, diag, seed):
    """{grad, loss_sums[, diag]} of one call of the layout's entry point on the handle's current arithmetic"""
    from uavppo import ops
    rs = np.random.RandomState(seed)
    D = 6 + k
    params = _dev(mlp_params(rs, D))
    s = samples(rs, N_TOTAL if layout == "rows" else n, D, factor)    # rows: the factor is on the upper half of the buffers
    rows = row_indices(rs, n) if layout == "rows" else None
    d = {key: _dev(v) for key, v in s.items()}
    args = [d[key] for key in ("act", "logp_old", "adv", "ret", "val_old")]
    sums = torch.full((4,), float("nan"), dtype=torch.float64, device=DEV)
    grad = torch.full_like(params, float("nan"))
    dbuf = torch.full((ops.PPO_DIAG_N,), float("nan"), dtype=torch.float64, device=DEV) if diag else None
    if diag:
        ops.set_ppo_diag(dbuf)
    try:
        if layout == "rows":
            ops.mlp_ppo_grad_rows(params, d["obs"], *args, _dev(rows), 1.0 / n, CLIP, BETA, sums, grad, k)
        elif k:
            ops.mlp_ppo_grad_trend(params, d["obs"], *args, 1.0 / n, CLIP, BETA, sums, grad, k)
        else:
            ops.mlp_ppo_grad(params, d["obs"], *args, 1.0 / n, CLIP, BETA, sums, grad)
        torch.cuda.synchronize()
    finally:
        if diag:
            ops.set_ppo_diag(None)
    out = {"grad": grad, "loss_sums": sums}
    if diag:
        out["diag"] = dbuf
    return out


def cases():
    """name -> (layout, arithmetic, trend_k); nothing here touches the GPU"""
    return {"%s-%s-k%d" % (layout, arith, k): (layout, arith, k)
            for layout in ("contig", "rows") for arith in ("fp16x3", "f32_mfma") for k in (0, 1, 2)}


def run_case(name):
    from uavppo import ops
    layout, arith, k = cases()[name]
    big = 2 * TILE * cu_count() + 7
    out = {}
    with ops.lstm_arith(arith):
        for i, (tag, n, factor, diag) in enumerate(RUNS):
            seed = 100 * sorted(cases()).index(name) + i
            for buf, v in run_one(layout, k, big if n is None else n, factor, diag, seed).items():
                assert torch.isfinite(v).all(), (name, tag, buf)
                out[tag + "." + buf] = _sha(v)
    return out


def main():
    out = {}
    for name in cases():
        out[name] = run_case(name)
        assert run_case(name) == out[name], f"{name}: two runs differ"
        print(f"{name}: {len(out[name])} buffers")
    path = sys.argv[1] if len(sys.argv) > 1 else PATH
    with open(path, "w") as f:
        json.dump({"cu_count": cu_count(), "cases": out}, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{path}: {len(out)} cases on {cu_count()} CUs, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
