"""The small f32 kernels behind offline training of the stop predictor (and under the layered MLP path), each called directly
through uavppo.ops and compared with a plain f64 reference written here: uav_ln_relu / uav_ln_relu_bwd, uav_smooth_l1,
uav_clip_adamw, uav_colsum.  Every input is generated in f32 and upcast for the reference, so input rounding is no error.

Two kinds of tolerance, no third:
  (a) a bound derived from the kernel's arithmetic, stated where it is used;
  (b) `check_b`: the error of the SAME operation in f32 torch on the CPU against f64 is the yardstick,
      err_kernel <= 2 * err_torch_f32 + 2 f32 ulps of the compared quantity's scale
      (2: the kernels reassociate sums -- wave shuffles, two-stage reductions -- where torch's CPU code does not).
Each (b) comparison prints its figures (pytest -s); the ratios measured on an MI355X are in MEASURED below.  -m gpu."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32, F64 = torch.float32, torch.float64
LN_EPS = 1e-5


@pytest.fixture(scope="module")
def ops():
    from uavppo import ops as o
    return o


def ulp32(x):
    """the spacing of f32 at |x|"""
    return float(np.spacing(np.float32(abs(float(x)))))


def check_b(name, got, want, ref32, scale=None):
    """Tolerance (b).  got: the kernel's result, want: f64, ref32: f32 torch on the CPU; all CPU tensors of one shape."""
    want = want.double()
    ek = float((got.double() - want).abs().max())
    et = float((ref32.double() - want).abs().max())
    floor = 2 * ulp32(float(want.abs().max()) if scale is None else scale)
    ratio = ek / et if et > 0 else float("inf") if ek > 0 else 0.0
    print(f"{name}: err_kernel {ek:.3e}  err_torch_f32 {et:.3e}  ratio {ratio:.2f}  floor {floor:.1e}")
    assert ek <= 2 * et + floor, (name, ek, et, floor)          # measured ratios: MEASURED below; a NaN in `got` fails here too
    return ratio


# MEASURED on an MI355X: err_kernel / err_torch_f32 of every check_b comparison, the largest over the row counts (LayerNorm) or
# over the five steps, both start steps and the three decays (AdamW).  Where the ratio is above 2 the error is a few ulps of
# a single element or row and sits under the 2-ulp floor (the f32 torch result happened to land closer), e.g. AdamW n = 1:
# param 6.3e-8 against torch's 3.0e-9 with a floor of 1.2e-7.
#   uav_ln_relu            cols   64    128    256    512        uav_ln_relu_bwd   cols   64    128    256    512
#     xhat                      1.09   1.05   1.37   1.53          dz (x row std)        0.77   1.30   1.08   2.15
#     a                         1.62   1.52   3.11   1.52          dgamma                1.59   0.83   0.91   1.10
#     rstd (relative)           1.29   1.42   3.17   1.00          dbeta                 1.09   1.18   1.14   1.17
#     |mean| / std = 1e3: xhat  0.68   0.83   0.73   0.83          exact masks: dgamma   0.54   1.16   1.01   2.40
#                         a     0.68   0.98   0.76   0.78
#                         rstd  0.00   0.01   0.01   0.01
#     (256: rows = 1 for a, rows = 4 for rstd; 512 dz and masks: rows = 5; every case with 2049 rows or more is below 1.2)
#   uav_clip_adamw         n       1   1023   1025   524291
#     param                    20.94   1.00   1.00   1.00
#     exp_avg                   1.01   1.46   1.54   1.05
#     exp_avg_sq               26.69   1.73   1.48   1.00
#   uav_colsum, err / bound (a): at most 0.035 (300 x 1024); 0.004 and 0.001 at 262,221 rows.


# ----------------------------------------------------------------------------- LayerNorm + ReLU
def ln_rows(rows, cols, seed, mean_over_std=None):
    """z [rows, cols] f32: every row has a scale of its own in 1e-3 .. 1e3 and a mean of up to 10 of its standard deviations
    (or of exactly +-mean_over_std of them)."""
    g = torch.Generator().manual_seed(seed)
    scale = 10.0 ** (torch.rand(rows, 1, generator=g, dtype=F64) * 6 - 3)
    u = torch.rand(rows, 1, generator=g, dtype=F64) * 2 - 1
    mean = (10 * u if mean_over_std is None else mean_over_std * torch.sign(u)) * scale
    return (mean + scale * torch.randn(rows, cols, generator=g, dtype=F64)).float(), g


def ln_f64(z):
    """(xhat, rstd) of LayerNorm(eps 1e-5) over the rows of z, in the arithmetic of z"""
    mean = z.mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((z - mean) ** 2).mean(1, keepdim=True) + LN_EPS)
    return (z - mean) * rstd, rstd[:, 0]


def ln_fwd_compare(ops, z, gam, bet, tag):
    z64 = z.double()
    xhat64, rstd64 = ln_f64(z64)
    a64 = torch.relu(F.layer_norm(z64, z.shape[1:], gam.double(), bet.double(), LN_EPS))
    assert torch.allclose(a64, torch.relu(xhat64 * gam.double() + bet.double()), rtol=1e-9, atol=1e-12)
    xhat32, _, rstd32 = torch.native_layer_norm(z, z.shape[1:], None, None, LN_EPS)      # f32 torch, the same operation
    a32 = torch.relu(F.layer_norm(z, z.shape[1:], gam, bet, LN_EPS))
    xh = z.to(DEV).clone()
    a, rstd = ops.ln_relu(xh, gam.to(DEV), bet.to(DEV), want_stats=True)
    check_b(f"ln_relu {tag} xhat", xh.cpu(), xhat64, xhat32)
    check_b(f"ln_relu {tag} a", a.cpu(), a64, a32)
    # rstd spans six decades over the rows: compared row by row at its own scale, i.e. as rstd / rstd_f64 against 1
    check_b(f"ln_relu {tag} rstd", rstd.cpu().double() / rstd64, torch.ones_like(rstd64), rstd32.reshape(-1).double() / rstd64)


# rows 16389 crosses the forward's 4096-block cap (4 rows a block): needed at the narrowest and the widest instantiation
LN_FWD_SHAPES = [(r, c) for c in (64, 128, 256, 512) for r in (1, 3, 4, 5, 2053)] + [(16389, 64), (16389, 512)]


@pytest.mark.parametrize("rows,cols", LN_FWD_SHAPES)
def test_ln_relu_forward_matches_f64(ops, rows, cols):
    """xhat, a and rstd by tolerance (b); measured ratios in MEASURED above."""
    z, g = ln_rows(rows, cols, seed=rows * 1000 + cols)
    gam = torch.randn(cols, generator=g)                    # about half of them negative
    bet = torch.randn(cols, generator=g)
    assert (gam < 0).any() and (gam > 0).any()
    ln_fwd_compare(ops, z, gam, bet, f"{rows}x{cols}")


@pytest.mark.parametrize("cols", [64, 128, 256, 512])
def test_ln_relu_forward_ill_conditioned_rows(ops, cols):
    """|mean| / std = 1e3: the mean's rounding error is 1e3 times larger against the spread; still tolerance (b)."""
    z, g = ln_rows(2053, cols, seed=77 + cols, mean_over_std=1e3)
    ln_fwd_compare(ops, z, torch.randn(cols, generator=g), torch.randn(cols, generator=g), f"ill 2053x{cols}")


@pytest.mark.parametrize("cols", [64, 128, 256, 512])
def test_ln_relu_forward_constant_and_nan_rows(ops, cols):
    rows = 9
    z, g = ln_rows(rows, cols, seed=cols)
    gam, bet = torch.randn(cols, generator=g).to(DEV), torch.randn(cols, generator=g).to(DEV)
    # constants of few significant bits: every partial sum of up to 512 of them is exact in f32, so the mean is the constant
    # itself, the centred row is exactly zero and rstd = 1 / sqrt(eps) (a constant with a full mantissa has an inexact f32
    # mean in any summation order, torch's included)
    consts = {1: 0.0, 4: -2.5, 6: 1000.125}
    for r, c in consts.items():
        z[r] = c
    xh = z.to(DEV).clone()
    a, rstd = ops.ln_relu(xh, gam, bet, want_stats=True)
    want_rstd = 1.0 / np.sqrt(LN_EPS)
    for r in consts:
        assert (xh[r] == 0).all(), r
        assert abs(float(rstd[r]) - want_rstd) <= ulp32(want_rstd), (r, float(rstd[r]))
        assert torch.equal(a[r], torch.relu(bet)), r
    # one NaN in a row: the whole row of `a` is NaN (torch.relu keeps NaN; the trainers' NaN check relies on it); the other rows
    # keep their bits
    z2 = z.clone()
    z2[3, cols // 2] = float("nan")
    xh2 = z2.to(DEV).clone()
    a2, rstd2 = ops.ln_relu(xh2, gam, bet, want_stats=True)
    assert torch.isnan(a2[3]).all() and torch.isnan(xh2[3]).all() and torch.isnan(rstd2[3])
    keep = [r for r in range(rows) if r != 3]
    assert torch.equal(a2[keep], a[keep]) and torch.equal(xh2[keep], xh[keep]) and torch.equal(rstd2[keep], rstd[keep])
    assert not torch.isnan(a[keep]).any()


def test_ln_relu_refuses_other_widths(ops):
    z = torch.randn(8, 96).to(DEV)
    z0 = z.clone()
    with pytest.raises(RuntimeError, match=r"uav_ln_relu failed \([1-9]\d*\).*width 96"):
        ops.ln_relu(z, torch.ones(96, device=DEV), torch.zeros(96, device=DEV))
    torch.cuda.synchronize()
    assert torch.equal(z, z0)
    d = z0.clone()
    dg, db = torch.full((96,), 7.0, device=DEV), torch.full((96,), 7.0, device=DEV)
    with pytest.raises(RuntimeError, match=r"uav_ln_relu_bwd failed \([1-9]\d*\).*width 96"):
        ops.ln_relu_bwd(d, z0, torch.ones(8, device=DEV), torch.ones(96, device=DEV), torch.zeros(96, device=DEV), dg, db)
    torch.cuda.synchronize()
    assert torch.equal(d, z0) and (dg == 7.0).all() and (db == 7.0).all()


def ln_bwd_run(ops, z, gam, bet, dy):
    """forward then backward on the device, as train_lstm.py chains them, twice: -> (dz, dgamma, dbeta) on the CPU"""
    cols = z.shape[1]
    xh = z.to(DEV).clone()
    _, rstd = ops.ln_relu(xh, gam.to(DEV), bet.to(DEV), want_stats=True)
    outs = []
    for garbage in (float("nan"), -3e30):                   # dgamma / dbeta are overwritten, not accumulated into
        d = dy.to(DEV).clone()
        dg, db = torch.full((cols,), garbage, device=DEV), torch.full((cols,), garbage, device=DEV)
        ops.ln_relu_bwd(d, xh, rstd, gam.to(DEV), bet.to(DEV), dg, db)
        outs.append((d.cpu(), dg.cpu(), db.cpu()))
    for x, y in zip(*outs):
        assert torch.equal(x, y)                             # two calls, the same bits
    return outs[0]


def ln_bwd_reference(z, gam, bet, dy, dtype):
    zz, gg, bb = (t.to(dtype).clone().requires_grad_(True) for t in (z, gam, bet))
    torch.relu(F.layer_norm(zz, z.shape[1:], gg, bb, LN_EPS)).backward(dy.to(dtype))
    return zz.grad, gg.grad, bb.grad


# rows 2049 and 2053 pass the backward's 512-block cap
@pytest.mark.parametrize("cols", [64, 128, 256, 512])
@pytest.mark.parametrize("rows", [1, 5, 2049, 2053])
def test_ln_relu_backward_matches_f64_autograd(ops, rows, cols):
    """dz, dgamma and dbeta by tolerance (b); measured ratios in MEASURED above."""
    z, g = ln_rows(rows, cols, seed=rows * 1000 + cols + 1)
    gam = 1 + 0.3 * torch.randn(cols, generator=g)
    bet = 0.3 * torch.randn(cols, generator=g)
    dy = torch.randn(rows, cols, generator=g)
    # An element whose pre-activation is within f32 error of 0 may get the other ReLU mask on the GPU, which moves dbeta by a
    # whole dy.  Nothing is left out of the comparison; the upstream gradient is zeroed there instead, so that either mask
    # gives the same answer.  At most 0.1 % of the elements may be affected (8e-5 to 9e-5 of them are, for these inputs).
    pre = F.layer_norm(z.double(), (cols,), gam.double(), bet.double(), LN_EPS)
    near = pre.abs() < 1e-4
    assert near.double().mean() <= 1e-3
    dy[near] = 0.0
    dz64, dg64, db64 = ln_bwd_reference(z, gam, bet, dy, F64)
    dz32, dg32, db32 = ln_bwd_reference(z, gam, bet, dy, F32)
    dz, dg, db = ln_bwd_run(ops, z, gam, bet, dy)
    std = 1.0 / ln_f64(z.double())[1][:, None]              # dz scales with 1 / std of its row: compared row by row, as dz * std
    tag = f"ln_relu_bwd {rows}x{cols}"
    check_b(f"{tag} dz", dz.double() * std, dz64 * std, dz32.double() * std)
    check_b(f"{tag} dgamma", dg, dg64, dg32)
    check_b(f"{tag} dbeta", db, db64, db32)


@pytest.mark.parametrize("cols", [64, 128, 256, 512])
def test_ln_relu_backward_exact_masks(ops, cols):
    """gamma = 0 makes the pre-activation exactly beta, so the mask is exact and needs no zeroing: beta = 0 and beta < 0 columns
    are masked (relu'(0) = 0 as in torch), beta > 0 columns pass and dbeta = sum of dy -- exactly, dy being small integers."""
    for rows in (5, 2053):
        z, g = ln_rows(rows, cols, seed=rows + cols)
        kind = torch.arange(cols) % 3                       # 0: beta = 0, 1: beta < 0, 2: beta > 0
        mag = 0.1 + torch.rand(cols, generator=g)
        bet = torch.where(kind == 0, torch.zeros(cols), torch.where(kind == 1, -mag, mag))
        gam = torch.zeros(cols)
        dy = torch.randint(-4, 5, (rows, cols), generator=g).float()
        dz, dg, db = ln_bwd_run(ops, z, gam, bet, dy)
        dz64, dg64, db64 = ln_bwd_reference(z, gam, bet, dy, F64)
        _, dg32, _ = ln_bwd_reference(z, gam, bet, dy, F32)
        assert (dz == 0).all() and (dz64 == 0).all()        # every dxhat = dy * gamma is 0
        masked = kind != 2
        assert (dg[masked] == 0).all() and (db[masked] == 0).all()
        assert torch.equal(db.double(), db64) and torch.equal(db64[~masked], dy.double().sum(0)[~masked])
        check_b(f"ln_relu_bwd masks {rows}x{cols} dgamma", dg, dg64, dg32)


# ----------------------------------------------------------------------------- SmoothL1
def smooth_l1_check(ops, pred, target, beta):
    n = pred.size
    d = pred - target                                       # f32, the one rounding the kernel makes too; f64 from here on
    dd = torch.tensor(d.astype(np.float64), requires_grad=True)
    want = F.smooth_l1_loss(dd, torch.zeros_like(dd), beta=beta)
    want.backward()
    want = float(want.detach())
    loss, dpred = ops.smooth_l1(torch.from_numpy(pred).to(DEV), torch.from_numpy(target).to(DEV), beta)
    loss, dpred, grad = float(loss.item()), dpred.cpu().numpy(), dd.grad.numpy()
    assert abs(loss - want) <= 1e-12 * abs(want), (loss, want)        # (a) the kernel sums in f64
    # (a) dpred = (d / beta) * f32(1 / n): beta is a power of two here, so two roundings (1 / n, the product) of at most
    # 2^-24 each against the exact quotient: 2^-23 |want| <= 2 ulps
    tol = 2 * np.spacing(np.abs(grad).astype(np.float32)).astype(np.float64)
    assert (np.abs(dpred.astype(np.float64) - grad) <= tol).all(), np.abs(dpred - grad).max()
    return loss, dpred


@pytest.mark.parametrize("beta", [0.5, 2.0])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
def test_smooth_l1_matches_f64(ops, n, beta):
    """n around the block's 256 threads (the loop's second pass starts at 257).  Planted: d = +-beta (the linear branch as in
    torch: gradient +-1/n), d = 0 (no loss, no gradient), |d| one ulp below beta (the quadratic branch)."""
    rng = np.random.RandomState(n)
    below = float(np.nextafter(np.float32(beta), np.float32(0)))
    planted = [beta, -beta, 0.0, below, -below]
    inv_n = np.float32(1) / np.float32(n)
    if n == 1:
        for dv in planted + [0.3 * beta, -3.0 * beta]:
            loss, dpred = smooth_l1_check(ops, np.array([dv], np.float32), np.zeros(1, np.float32), beta)
            if abs(dv) == beta:
                assert dpred[0] == np.sign(dv) * inv_n and loss == 0.5 * beta
            if dv == 0:
                assert dpred[0] == 0 and loss == 0
        return
    target = rng.randn(n).astype(np.float32)
    pred = (target + 1.5 * beta * rng.randn(n)).astype(np.float32)
    where = [0, 1, n // 2, n - 2, n - 1]                  # the last two in the second pass when n > 256
    for i, dv in zip(where, planted):
        target[i], pred[i] = 0.0, dv
    a = np.abs(pred - target)
    assert (a < beta).sum() > n // 4 and (a > beta).sum() > n // 4          # both branches well populated
    _, dpred = smooth_l1_check(ops, pred, target, beta)
    assert dpred[0] == inv_n and dpred[1] == -inv_n and dpred[n // 2] == 0


@pytest.mark.parametrize("n,k", [(1, 0), (300, 0), (300, 299)])
def test_smooth_l1_nan_reaches_loss_and_gradient(ops, n, k):
    """A NaN prediction gives a NaN loss AND a NaN gradient at that element (torch does; a finite -1/n there would hide it
    from anything that looks at the gradient alone); the other elements keep their gradients."""
    rng = np.random.RandomState(5)
    target = rng.randn(n).astype(np.float32)
    pred = (target + rng.randn(n)).astype(np.float32)
    _, clean = ops.smooth_l1(torch.from_numpy(pred).to(DEV), torch.from_numpy(target).to(DEV), 1.0)
    pred[k] = np.nan
    loss, dpred = ops.smooth_l1(torch.from_numpy(pred).to(DEV), torch.from_numpy(target).to(DEV), 1.0)
    t = torch.tensor(pred.astype(np.float64), requires_grad=True)
    F.smooth_l1_loss(t, torch.from_numpy(target).double(), beta=1.0).backward()
    assert torch.isnan(t.grad[k])                           # the reference's behaviour
    assert torch.isnan(loss).all() and torch.isnan(dpred[k])
    others = [i for i in range(n) if i != k]
    assert torch.equal(dpred[others], clean[others])


# ----------------------------------------------------------------------------- clip + AdamW
def f32r(x):
    """a hyper-parameter as the f32 the C ABI receives, so that its rounding is no error"""
    return float(np.float32(x))


ADAM = dict(lr=f32r(1e-3), beta1=f32r(0.9), beta2=f32r(0.999), eps=f32r(1e-8))


class TorchAdamW:
    """torch.optim.AdamW(foreach=False) + clip_grad_norm_ on the CPU in `dtype`, started at optimiser step `step0`."""

    def __init__(self, p0, m0, v0, step0, weight_decay, max_norm, dtype):
        self.p = torch.nn.Parameter(p0.to(dtype).clone())
        self.opt = torch.optim.AdamW([self.p], lr=ADAM["lr"], betas=(ADAM["beta1"], ADAM["beta2"]), eps=ADAM["eps"],
                                     weight_decay=weight_decay, foreach=False)
        self.opt.state[self.p] = {"step": torch.tensor(float(step0 - 1)), "exp_avg": m0.to(dtype).clone(),
                                  "exp_avg_sq": v0.to(dtype).clone()}
        self.max_norm, self.dtype = max_norm, dtype

    def step(self, g):
        self.p.grad = g.to(self.dtype).clone()
        if self.max_norm > 0:
            norm = torch.nn.utils.clip_grad_norm_([self.p], self.max_norm)
        else:
            norm = self.p.grad.norm()
        self.opt.step()
        st = self.opt.state[self.p]
        return float(norm), self.p.detach(), st["exp_avg"], st["exp_avg_sq"]


def adamw_inputs(n, step0, seed):
    g = torch.Generator().manual_seed(seed)
    p0 = torch.randn(n, generator=g)
    if step0 == 1:
        m0, v0 = torch.zeros(n), torch.zeros(n)
    else:                                                   # a state as it is late in a run
        m0 = 0.05 * torch.randn(n, generator=g)
        v0 = (0.05 * torch.randn(n, generator=g)) ** 2 + 1e-6
    # five steps, alternately clipped (norm > 1) and unclipped
    grads = [torch.randn(n, generator=g) * (3.0 if s % 2 == 0 else 1e-3) for s in range(5)]
    return p0, m0, v0, grads


def adamw_compare(ops, n, weight_decay, step0, max_norm, tag, steps=5):
    p0, m0, v0, grads = adamw_inputs(n, step0, seed=n + step0)
    ref64 = TorchAdamW(p0, m0, v0, step0, weight_decay, max_norm, F64)
    ref32 = TorchAdamW(p0, m0, v0, step0, weight_decay, max_norm, F32)
    p, m, v = p0.to(DEV), m0.to(DEV), v0.to(DEV)
    gn = torch.zeros(1, device=DEV)
    worst = {"param": 0.0, "exp_avg": 0.0, "exp_avg_sq": 0.0}
    for s, g in enumerate(grads[:steps]):
        norm64, *want = ref64.step(g)
        _, *t32 = ref32.step(g)
        ops.clip_adamw(p, g.to(DEV), m, v, step0 + s, weight_decay=weight_decay, max_norm=max_norm, gnorm_out=gn, **ADAM)
        assert abs(gn.item() - norm64) <= 1e-6 * norm64, (s, gn.item(), norm64)
        for name, got, w, t in zip(worst, (p, m, v), want, t32):
            worst[name] = max(worst[name], check_b(f"clip_adamw {tag} step {step0 + s} {name}", got.cpu(), w, t))
    print(f"clip_adamw {tag}: worst ratios {worst}")


# n = 524291 crosses both caps: more than 256 * 1024 elements for the norm's partial sums, more than 2048 * 256 for the step
@pytest.mark.parametrize("step0", [1, 100000])
@pytest.mark.parametrize("weight_decay", [0.0, f32r(1e-4), f32r(0.1)])
@pytest.mark.parametrize("n", [1, 1023, 1025, 524291])
def test_clip_adamw_matches_f64_torch(ops, n, weight_decay, step0):
    """Five steps, gnorm_out to 1e-6, param and both moments by tolerance (b) after each; measured ratios in MEASURED above."""
    adamw_compare(ops, n, weight_decay, step0, 1.0, f"n={n} wd={weight_decay:g} step0={step0}")


@pytest.mark.parametrize("max_norm", [0.0, -1.0])
def test_clip_adamw_max_norm_not_positive_disables_clipping(ops, max_norm):
    adamw_compare(ops, 1025, f32r(0.1), 1, max_norm, f"max_norm={max_norm:g}", steps=2)


@pytest.mark.parametrize("n", [1, 1025, 524291])
def test_clip_adamw_without_decay_equals_clip_adam(ops, n):
    p0, m0, v0, grads = adamw_inputs(n, 100000, seed=n)
    a = [t.to(DEV).clone() for t in (p0, m0, v0)] + [torch.zeros(1, device=DEV)]
    b = [t.to(DEV).clone() for t in (p0, m0, v0)] + [torch.zeros(1, device=DEV)]
    for s, g in enumerate(grads[:2]):
        ops.clip_adamw(a[0], g.to(DEV), a[1], a[2], 7 + s, weight_decay=0.0, max_norm=1.0, gnorm_out=a[3], **ADAM)
        ops.clip_adam(b[0], g.to(DEV), b[1], b[2], 7 + s, max_norm=1.0, gnorm_out=b[3], **ADAM)
        for x, y in zip(a, b):
            assert torch.equal(x, y)


@pytest.mark.parametrize("n", [1, 1025])
def test_clip_adamw_zero_and_nan_gradients(ops, n):
    p0 = torch.randn(n, generator=torch.Generator().manual_seed(n))
    wd = f32r(0.1)
    p, m, v, gn = p0.to(DEV).clone(), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV), torch.ones(1, device=DEV)
    ops.clip_adamw(p, torch.zeros(n, device=DEV), m, v, 1, weight_decay=wd, max_norm=1.0, gnorm_out=gn, **ADAM)
    # (a) the moments stay 0 and 0 / (0 + eps) = 0: what is left is the decay, p * f32(1 - f32(lr * wd)), one rounding
    decay = np.float32(1) - np.float32(ADAM["lr"]) * np.float32(wd)
    assert gn.item() == 0 and (m == 0).all() and (v == 0).all()
    assert np.array_equal(p.cpu().numpy(), p0.numpy() * decay) and decay < 1
    # a NaN gradient: the norm the host reads back is NaN (its only signal)
    g = torch.zeros(n)
    g[n // 2] = float("nan")
    ops.clip_adamw(p, g.to(DEV), m, v, 2, weight_decay=wd, max_norm=1.0, gnorm_out=gn, **ADAM)
    assert torch.isnan(gn).all()


# ----------------------------------------------------------------------------- column sums
def colsum_chain(rows, cols, vec):
    """(a) The longest chain of f32 additions one element passes through on its way into out[c], read off csrc/mlp.hip.
    colsum_absmax: nb = min(ceil(rows / 256), 1024) blocks of rpb = ceil(rows / nb) rows (so rpb > 256 from 262,145 rows on).
    colsum_partial_kernel (scalar path): one accumulator takes the block's rpb rows in turn: rpb additions.
    colsum_partial4_kernel (cols % 4 == 0 and a 16-byte aligned base): row i of the block goes to accumulator i % 4, the
    rpb % 4 left-over rows to accumulator 0, then (a0 + a1) + (a2 + a3): rpb // 4 + rpb % 4 + 2 additions.
    rows_reduce_kernel: partial b goes to accumulator b % 8 over whole groups of 8, the nb % 8 left over to accumulator 0, then
    a three-level tree: nb // 8 + nb % 8 + 3 additions.  (The additions onto a zero accumulator are exact; counting them keeps
    the bound safe.)  Each addition's rounding error is at most 2^-24 of its result, which is at most sum |x|, so
    |out[c] - sum_r x[r][c]| <= k * 2^-24 * sum_r |x[r][c]| (to first order in 2^-24; k 2^-24 < 3e-5 here)."""
    nb = min((rows + 255) // 256, 1024)
    rpb = (rows + nb - 1) // nb
    nb = (rows + rpb - 1) // rpb
    partial = rpb // 4 + rpb % 4 + 2 if vec else rpb
    return partial + nb // 8 + nb % 8 + 3


def colsum_check(ops, x, vec):
    rows, cols = x.shape
    assert (x.data_ptr() % 16 == 0 and cols % 4 == 0) == vec
    xc = x.cpu().double()
    got = ops.colsum(x)
    assert torch.equal(ops.colsum(x), got)                  # two calls, the same bits
    err = (got.cpu().double() - xc.sum(0)).abs()
    bound = colsum_chain(rows, cols, vec) * 2.0 ** -24 * xc.abs().sum(0)
    assert (err <= bound).all(), (float((err / bound.clamp_min(1e-300)).max()), colsum_chain(rows, cols, vec))
    return float((err / bound.clamp_min(1e-300)).max())


COLSUM_SHAPES = [(1, 1), (255, 3), (257, 2), (300, 1023), (300, 1024), (1000, 64), (262221, 4), (262221, 3)]


@pytest.mark.parametrize("rows,cols", COLSUM_SHAPES)
def test_colsum_within_its_rounding_bound(ops, rows, cols):
    g = torch.Generator().manual_seed(rows + cols)
    x = (0.5 + torch.randn(rows, cols, generator=g)).to(DEV)          # a mean, so that the sums grow with the rows
    print(f"colsum {rows}x{cols}: err / bound {colsum_check(ops, x, cols % 4 == 0):.3f}")
    # small integers: every partial sum is an integer below 2^24, so every addition is exact in any association and the
    # bound (a) shrinks to equality -- one dropped or doubled row anywhere shows, also among 262,221 of them
    xi = torch.randint(-8, 9, (rows, cols), generator=g).float().to(DEV)
    assert torch.equal(ops.colsum(xi).cpu().double(), xi.cpu().double().sum(0))


def test_colsum_unaligned_base_takes_the_scalar_path(ops):
    """cols = 64 but the matrix starts one float into a buffer: not 16-byte aligned, so no dwordx4 loads."""
    rows, cols = 1000, 64
    g = torch.Generator().manual_seed(1)
    buf = (0.5 + torch.randn(rows * cols + 1, generator=g)).to(DEV)
    x = buf[1:].view(rows, cols)
    assert x.is_contiguous() and x.data_ptr() % 16 == 4
    colsum_check(ops, x, vec=False)
    bi = torch.randint(-8, 9, (rows * cols + 1,), generator=g).float().to(DEV)
    xi = bi[1:].view(rows, cols)
    assert torch.equal(ops.colsum(xi).cpu().double(), xi.cpu().double().sum(0))


def test_colsum_refuses_more_than_1024_columns(ops):
    out = torch.full((1025,), 7.0, device=DEV)
    with pytest.raises(RuntimeError, match=r"uav_colsum failed \([1-9]\d*\)"):
        ops.colsum(torch.ones(4, 1025, device=DEV), out=out)
    torch.cuda.synchronize()
    assert (out == 7.0).all()
