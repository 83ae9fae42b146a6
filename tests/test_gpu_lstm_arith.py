"""The h = 64 / 128 LSTM layer in each of its three arithmetics (uav_set_lstm_arith) against an f64 LSTM, at the shapes that
pick each of its kernels: forward, backward and weight gradients, every output of the layer.

    fp16x3    the default: 16-bit matrix pipe, f32 operands split into two fp16 pieces (common.h SplitF16x3, wgrad.hip WgF16x3)
    bf16x6    what the trainer's range guard switches to (uavppo/trainer.py RANGE_LIMITS): three bf16 pieces, six products,
              f32's exponent range (SplitBf16x6, WgBf16x6)
    f32_mfma  the exact-f32 MFMA kernels: the yardstick of the other two

Criterion of the suite (test_gpu_lstm.py, test_split_kernels_have_f32_accuracy): against f64, e = max|G - R| / max|R| below
5e-6 in every mode, and each split mode no worse than twice the exact-f32 kernels' error + 2e-7.  -m gpu."""
import pytest
import torch

from oracle import ppo_oracle as po

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64 = torch.float64
MODES = ("fp16x3", "bf16x6", "f32_mfma")
SPLITS = ("fp16x3", "bf16x6")


@pytest.fixture(scope="module")
def ops():
    from uavppo import ops as o
    return o


# ---- the dispatch rules of the h = 64 / 128 layer, restated (a case's kernels follow from its shape, heads and mode):
#   forward   csrc/lstm_api.hip (uav_lstm_fwd)  I <= 8: the input product fused into the sequence kernel; I > 8: a GEMM into the
#             stash first.  lstm.hip launch_fwd: the split kernels (heads fused) unless f32_mfma, then the exact kernel + one heads GEMM.
#   backward  csrc/lstm.hip lstm_bwd_seq  dheads with at most 7 heads and not f32_mfma: the split kernel (lstm_bwd_split);
#             else (8 heads, plain dy, f32_mfma) the exact kernel (lstm_bwd_kernel).
#   wgrad     csrc/lstm_api.hip (uav_lstm_wgrad)  I <= 6: launch_wgrad (csrc/wgrad.hip), else column sums + products (LstmWgrad::rows).
#             wgrad.hip:632-645: nb = min(num_cu, workspace / slab); rows per block rounded up to 16, nb refitted; rpx = the
#             rows per block rounded up to 32; the split kernel iff N T % rpx == 0, T >= 8, I <= 6, at most 8 heads,
#             N T 4H < 2^30 and not f32_mfma (rpx / 32 slabs per workgroup), else the exact kernel lstm_wgrad_kernel.
#             The split kernel stages h_prev in groups of 8 rows: a sequence start that is not the first row of its group
#             (wgrad.hip:405, only when T % 8 != 0) takes h0 in place of the previous env's last y.
def wgrad_split_slabs(N, T, I, H, NH, num_cu, ws_bytes):
    """Slabs per workgroup of the split weight-gradient kernel on a split arithmetic, 0 where the exact kernel runs."""
    slab_bytes = (4 * H * (H + 16) + 16 * H) * 4                     # WG<H>::SLAB floats
    NT = N * T
    nb = min(num_cu, ws_bytes // slab_bytes)
    rpb = -(-NT // nb)
    rpb = -(-rpb // 16) * 16
    nb = -(-NT // rpb)
    rpx = -(-NT // nb)
    rpx = -(-rpx // 32) * 32
    ok = NT % rpx == 0 and T >= 8 and I <= 6 and NH <= 8 and NT * 4 * H < (1 << 30)
    return rpx // 32 if ok else 0


def kernel_classes(N, T, I, H, NH, num_cu, ws_bytes):
    """The kernels a case runs on the two split arithmetics (f32_mfma runs the exact kernels throughout)."""
    fwd = "fused" if I <= 8 else "unfused"
    bwd = ("split" if NH <= 7 else "exact") if NH else "exact-dy"
    if I > 6:
        wg = "colsum+product" if I <= 8 else "products"
    else:
        s = wgrad_split_slabs(N, T, I, H, NH, num_cu, ws_bytes)
        wg = f"split/{s}-slab" + ("/T%8" if T % 8 else "") if s else "exact"
    return fwd, bwd, wg


def device_geometry(ops):
    return torch.cuda.get_device_properties(0).multi_processor_count, ops.WS_BYTES


# (H, N, T, I, heads (None: plain dy), keep): restart masks "none" (no mask), "rand" (restarts inside the sequences),
# "start0" (as rand, and every third env restarts at t = 0), "zerocol" (as rand, and every env restarts at t = T // 2).
# On 256 CUs the split weight-gradient kernel takes T % 8 != 0 at (32, 9), (8, 12), (40, 12), (64, 15), (32, 33), (32, 10),
# (768, 12) -- the last with two slabs per workgroup; test_matrix_covers_every_kernel_class checks that on the device.
CASES = [
    (64, 1, 1, 6, 6, "none"),              # T = 1, one env
    (128, 5, 3, 1, 1, "start0"),           # T < 8: exact wgrad; I = 1, one head
    (64, 17, 7, 6, 7, "rand"),             # T < 8, 7 heads
    (128, 37, 21, 6, 7, "zerocol"),        # N T not a multiple of the slab rows: exact wgrad
    (64, 40, 24, 6, 8, "rand"),            # 8 heads: exact backward with dheads, split wgrad with 8 heads
    (128, 32, 9, 6, 6, "start0"),          # split wgrad, T % 8 != 0 ...
    (64, 8, 12, 6, 6, "rand"),
    (128, 40, 12, 6, 1, "start0"),
    (64, 64, 15, 6, 7, "zerocol"),
    (128, 64, 15, 6, 6, "start0"),
    (128, 32, 33, 6, 6, "rand"),
    (64, 32, 33, 6, 6, "start0"),
    (128, 768, 12, 6, 6, "start0"),        # ... with two slabs per workgroup
    (64, 768, 12, 6, None, "rand"),        # plain dy, two slabs per workgroup
    (128, 16, 16, 6, None, "none"),        # plain dy, whole env tiles, T % 8 == 0
    (64, 32, 10, 6, None, "start0"),       # plain dy, split wgrad T % 8 != 0
    (64, 64, 15, 1, None, "rand"),         # plain dy, I = 1
    (128, 16, 64, 6, 6, "rand"),           # split wgrad, T % 8 == 0
    (128, 48, 32, 8, 6, "rand"),           # I = 8: fused forward, column-sum pass + product
    (64, 17, 10, 7, 8, "start0"),          # I = 7, 8 heads
    (128, 5, 33, 8, 1, "rand"),
    (64, 5, 9, 40, 6, "rand"),             # I > 8: input GEMM into the stash, products, dx
    (128, 37, 12, 128, None, "zerocol"),
    (128, 40, 8, 40, 8, "start0"),
    (64, 16, 6, 128, 7, "rand"),
    (64, 1, 40, 6, 6, "rand"),             # one env, 40 rows: exact wgrad
    (128, 1, 8, 1, 6, "none"),             # 8 rows: exact wgrad
    (64, 100, 5, 6, 6, "zerocol"),         # T < 8
]


def _case_id(c):
    H, N, T, I, NH, keep = c
    return f"H{H}-N{N}-T{T}-I{I}-{'dy' if NH is None else f'nh{NH}'}-{keep}"


def make_problem(H, N, T, I, NH, keep_mode, seed):
    """One layer problem in f64, time-major as the oracle takes it; every quantity O(1) across envs and steps, and each
    exactly representable in f32."""
    g = torch.Generator().manual_seed(seed)
    k = H ** -0.5
    u = lambda *s: (torch.rand(*s, generator=g, dtype=F64) * 2 - 1) * k
    n = lambda *s, sc=1.0: torch.randn(*s, generator=g, dtype=F64) * sc
    A = NH or 6
    p = {"w_ih": u(4 * H, I), "w_hh": u(4 * H, H), "b_ih": u(4 * H), "b_hh": u(4 * H),
         "x": n(T, N, I), "h0": n(N, H, sc=0.5), "c0": n(N, H, sc=0.5), "w_head": n(A, H, sc=0.3), "b_head": n(A, sc=0.1),
         "dhn": n(N, H, sc=0.5), "dcn": n(N, H, sc=0.5)}
    if NH:
        p["dheads"] = n(T, N, NH)
    else:
        p["dy"] = n(T, N, H, sc=0.5)
    keep = None
    if keep_mode != "none":
        keep = (torch.rand(T, N, generator=g) > 0.15).double()
        keep[0] = 1.0
        if keep_mode == "start0":
            keep[0, ::3] = 0.0
        elif keep_mode == "zerocol":
            keep[T // 2] = 0.0
    p = {k: v.float().double() for k, v in p.items()}                           # the f32 values the kernels are given
    p["keep"] = keep
    return p


def oracle(p):
    """f64 forward + autograd: y, hn, cn, heads and the gradients of (heads . dheads | y . dy) + hn . dhn + cn . dcn."""
    leaf = {k: p[k].clone().requires_grad_(True) for k in ("x", "h0", "c0", "w_ih", "w_hh", "b_ih", "b_hh", "w_head")}
    y, hn, cn = po.lstm_layer_forward(leaf["x"], leaf["h0"], leaf["c0"], leaf["w_ih"], leaf["w_hh"], leaf["b_ih"], leaf["b_hh"],
                                      p["keep"])
    heads = y @ leaf["w_head"].T + p["b_head"]
    loss = (heads * p["dheads"]).sum() if "dheads" in p else (y * p["dy"]).sum()
    (loss + (hn * p["dhn"]).sum() + (cn * p["dcn"]).sum()).backward()
    want = {"y": y.transpose(0, 1), "hn": hn, "cn": cn, "heads": heads.transpose(0, 1), "dx": leaf["x"].grad.transpose(0, 1),
            "dw_ih": leaf["w_ih"].grad, "dw_hh": leaf["w_hh"].grad, "db": leaf["b_ih"].grad, "dh0": leaf["h0"].grad,
            "dc0": leaf["c0"].grad}
    if "dheads" in p:
        want["dw_head"] = leaf["w_head"].grad
    return {k: v.detach() for k, v in want.items()}


def run_layer(ops, p, mode):
    """The product through uavppo.ops alone (forward with heads, backward with dx, weight gradients) in one arithmetic."""
    d = lambda t: None if t is None else t.detach().float().to(DEV).contiguous()
    em = lambda t: None if t is None else d(t.transpose(0, 1))                        # time-major -> env-major
    x, keep = em(p["x"]), em(p["keep"])
    w_ih, w_hh, b_ih, b_hh, h0, c0 = (d(p[k]) for k in ("w_ih", "w_hh", "b_ih", "b_hh", "h0", "c0"))
    w_head = d(p["w_head"])
    N, T, _ = x.shape
    with ops.lstm_arith(mode):
        heads = torch.full((N, T, w_head.shape[0]), float("nan"), device=DEV)
        y, hn, cn, stash = ops.lstm_fwd(x, keep, h0, c0, w_ih, w_hh, b_ih, b_hh, w_head=w_head, b_head=d(p["b_head"]), heads=heads)
        if "dheads" in p:
            g = ops.lstm_bwd(x, keep, stash, w_ih, w_hh, y, h0, dheads=em(p["dheads"]), w_head=w_head, dhn=d(p["dhn"]),
                             dcn=d(p["dcn"]), need_dx=True)
        else:
            g = ops.lstm_bwd(x, keep, stash, w_ih, w_hh, y, h0, dy=em(p["dy"]), dhn=d(p["dhn"]), dcn=d(p["dcn"]), need_dx=True)
    g.update(y=y, hn=hn, cn=cn, heads=heads)
    return g


def rel_errors(ops, p, want):
    out = {}
    for mode in MODES:
        got = run_layer(ops, p, mode)
        out[mode] = {k: float((got[k].double().cpu() - w).abs().max() / w.abs().max()) for k, w in want.items()}
    assert ops.get_lstm_arith() == "fp16x3"
    return out


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_layer_in_every_arithmetic_matches_f64(ops, case):
    """Every output of the layer against the f64 LSTM, once per arithmetic: the oracle is computed once and shared."""
    H, N, T, I, NH, keep = case
    p = make_problem(*case, seed=1000 + CASES.index(case))
    want = oracle(p)
    e = rel_errors(ops, p, want)
    print(_case_id(case), {m: f"{max(e[m].values()):.2e} ({max(e[m], key=e[m].get)})" for m in MODES})
    # every miss of every mode in one message
    bad = [(m, k, e[m][k]) for m in MODES for k in want if not e[m][k] < 5e-6]                 # f32-level agreement with f64
    bad += [(m, k, e[m][k], e["f32_mfma"][k]) for m in SPLITS for k in want if not e[m][k] <= 2.0 * e["f32_mfma"][k] + 2e-7]
    assert not bad, bad


# ---- the split weight gradient alone, at sequence starts inside an 8-row group (T % 8 != 0), one and several slabs per
# workgroup, with and without heads: (N, T, H)
WGRAD_CASES = [(32, 9, 128), (8, 12, 64), (40, 12, 128), (64, 15, 64), (32, 33, 128), (768, 12, 64), (768, 12, 128),
               (2048, 100, 128)]


def _row_rel(got, want):
    """Per row, the largest error against that row's own largest magnitude."""
    return (got - want).abs().amax(1) / want.abs().amax(1).clamp_min(1e-300)


@pytest.mark.parametrize("heads", [False, True])
@pytest.mark.parametrize("N,T,H", WGRAD_CASES)
def test_split_wgrad_takes_h0_at_sequence_starts_inside_a_group(ops, N, T, H, heads):
    """uav_lstm_wgrad from given gate gradients, h0 drawn independently of y: a start row's h_prev (h0 of ITS env, times
    keep) differs from the row before it (y of the previous env's last step).  dW_hh, dW_ih, dW_head per gate row, db
    against its sum of magnitudes, all against f64 sums of exactly the f32 operands the kernel is given -- under both
    split arithmetics (the split kernel on these shapes) and f32_mfma (the exact kernel, their yardstick)."""
    I = 6
    num_cu, ws = device_geometry(ops)
    assert T % 8 and wgrad_split_slabs(N, T, I, H, 6 if heads else 0, num_cu, ws) >= 1
    g = torch.Generator().manual_seed(N * 1000 + T * 10 + H + heads)
    f32 = lambda t: t.float().double()                                         # the values the kernel sees
    x = f32(torch.rand(N, T, I, generator=g, dtype=F64) * 2 - 1)
    y = f32(torch.rand(N, T, H, generator=g, dtype=F64) * 2 - 1)
    h0 = f32(torch.rand(N, H, generator=g, dtype=F64) * 2 - 1)
    keep = (torch.rand(N, T, generator=g) > 0.1).double()
    keep[:, 0] = 1.0
    keep[::9, 0] = 0.0                                                         # a few envs restart at t = 0
    dg = f32(torch.randn(N, T, 4 * H, generator=g, dtype=F64))
    dheads = f32(torch.randn(N, T, 6, generator=g, dtype=F64)) if heads else None
    hprev = torch.cat([h0[:, None], y[:, :-1]], 1) * keep[..., None]
    # f64 sums on the device (ordinary f64 GEMMs: at N T = 204,800 rows the host would take a while)
    dd = lambda t: t.to(DEV).reshape(N * T, -1)
    want = {"dw_hh": dd(dg).T @ dd(hprev), "dw_ih": dd(dg).T @ dd(x)}
    want_b, abs_b = dd(dg).sum(0), dd(dg).abs().sum(0)
    if heads:
        want["dw_head"] = dd(dheads).T @ dd(y)
    d = lambda t: t.float().to(DEV).contiguous()
    stash = torch.zeros(N, T, 6 * H, device=DEV)                               # not read on the I <= 6 path
    row, berr = {}, {}
    for mode in MODES:
        with ops.lstm_arith(mode):
            got = ops.lstm_wgrad(d(x), d(keep), d(h0), d(y), stash, d(dg), torch.zeros(4 * H, I, device=DEV),
                                 dheads=d(dheads) if heads else None)
        row[mode] = {k: _row_rel(got[k].double(), w) for k, w in want.items()}
        berr[mode] = float(((got["db"].double() - want_b).abs() / abs_b).max())
    assert ops.get_lstm_arith() == "fp16x3"
    worst = {m: {k: float(v.max()) for k, v in row[m].items()} for m in MODES}
    print(N, T, H, heads, worst, berr)
    bad = [(m, k, worst[m][k]) for m in MODES for k in want if not worst[m][k] < 5e-6]
    bad += [(m, "db", berr[m]) for m in MODES if not berr[m] < 3e-7]
    bad += [(m, k, worst[m][k], worst["f32_mfma"][k]) for m in SPLITS for k in want
            if not worst[m][k] <= 2.0 * worst["f32_mfma"][k] + 2e-7]
    assert not bad, bad


# ---- bf16x6 where fp16x3 cannot go: operands beyond the fp16 split's range (trainer.py RANGE_LIMITS: |w| < 65504,
# |x| < 4096, |h0| < 64), per env and per gate row against f64, the exact-f32 kernels on the same case as the yardstick
def _per_row(got, want):
    """Per env (leading axis) or gate row: largest error against that slice's largest magnitude; the worst slice."""
    g, w = got.double().cpu().reshape(got.shape[0], -1), want.reshape(want.shape[0], -1)
    return float(_row_rel(g, w).max())


@pytest.mark.parametrize("operand", ["w_hh", "x_fused", "x_wide", "h0"])
def test_bf16x6_beyond_the_fp16_range_matches_f64(ops, operand):
    """Recurrent weights of 1e5, inputs up to 3e4 (on the fused-input and on the I > 8 path), |h0| = 100 in some units --
    each paired with small weights on the other side of its product, so that every gate stays O(1) and the problem keeps
    its conditioning: a wrong piece shows as error, not as saturation.  bf16x6 per env (y, hn, cn, heads, dx, dh0, dc0)
    and per gate row (dW_ih, dW_hh, dW_head; db as a whole) below 5e-6 of the slice's magnitude and no worse than twice
    the exact-f32 kernels' worst slice + 2e-7.  40 envs x 12 steps: a partial env tile, and the split weight-gradient
    kernel with sequence starts inside its 8-row groups."""
    H, N, T, NH = 128, 40, 12, 6
    I = 40 if operand == "x_wide" else 6
    p = make_problem(H, N, T, I, NH, "start0", seed=77)
    if operand == "w_hh":
        # four units kept tiny (output gate bias -12: |h| < 2e-5) drive gate rows of four other units through weights of 1e5
        U = torch.tensor([5, 17, 64, 100])
        p["b_ih"][3 * H + U] = -12.0
        p["h0"][:, U] *= 1e-5
        p["w_hh"][torch.tensor([3, 200, 300, 450]), U] = torch.tensor([1e5, -1e5, 1e5, -1e5], dtype=F64)
    elif operand in ("x_fused", "x_wide"):
        # (every column: a row of dW_ih with one wide column is a sum that cancels to 1e-3 of its terms in some rows)
        p["x"] = (p["x"] * 1e4).clamp(-3e4, 3e4).float().double()                    # past 4096 in most rows
        p["w_ih"] = (p["w_ih"] * 1e-4).float().double()
    else:
        p["h0"][:, 8:16] = 100.0 * torch.sign(p["h0"][:, 8:16])
        p["w_hh"][:, 8:16] = (p["w_hh"][:, 8:16] * 1e-2).float().double()
    assert float(max(p["w_hh"].abs().max(), p["x"].abs().max(), p["h0"].abs().max())) > 64.0
    want = oracle(p)
    num_cu, ws = device_geometry(ops)
    if I <= 6:
        assert wgrad_split_slabs(N, T, I, H, NH, num_cu, ws) >= 1
    err = {}
    for mode in ("bf16x6", "f32_mfma"):
        got = run_layer(ops, p, mode)
        for k in want:
            assert torch.isfinite(got[k]).all(), (mode, k)
        err[mode] = {k: (float((got[k].double().cpu() - w).abs().max() / w.abs().max()) if k == "db" else _per_row(got[k], w))
                     for k, w in want.items()}
    assert ops.get_lstm_arith() == "fp16x3"
    print(operand, err)
    for k in want:
        assert err["bf16x6"][k] < 5e-6, (k, err)
        assert err["bf16x6"][k] <= 2.0 * err["f32_mfma"][k] + 2e-7, (k, err)


def test_matrix_covers_every_kernel_class(ops):
    """The matrices above were built from the dispatch rules on 256 CUs: on the device this runs on, they must still reach
    every kernel class -- a different CU count or workspace fails here instead of silently dropping a path."""
    num_cu, ws = device_geometry(ops)
    seen = set()
    for c in CASES:
        H, N, T, I, NH, keep = c
        fwd, bwd, wg = kernel_classes(N, T, I, H, NH or 0, num_cu, ws)
        print(f"{_case_id(c):32s} fwd {fwd:8s} bwd {bwd:9s} wgrad {wg}")
        seen |= {"fwd-" + fwd, "bwd-" + bwd, "wgrad-" + wg.split("/")[0]}
        if wg.startswith("split") and T % 8:
            seen.add("wgrad-split-T%8")
        if wg.startswith("split") and not wg.startswith("split/1-"):
            seen.add("wgrad-split-multislab")
        if N % 16:
            seen.add("partial-env-tile")
    want = {"fwd-fused", "fwd-unfused", "bwd-split", "bwd-exact", "bwd-exact-dy", "wgrad-split", "wgrad-exact",
            "wgrad-colsum+product", "wgrad-products", "wgrad-split-T%8", "wgrad-split-multislab", "partial-env-tile"}
    assert want <= seen, (num_cu, ws, want - seen)
    for N, T, H in WGRAD_CASES:
        for nh in (0, 6):
            assert wgrad_split_slabs(N, T, 6, H, nh, num_cu, ws) >= 1, (N, T, H, nh, num_cu)
    assert any(wgrad_split_slabs(N, T, 6, H, 0, num_cu, ws) > 1 for N, T, H in WGRAD_CASES)
