"""The small kernels every optimiser step runs through, each called directly through uavppo.ops and compared with an f64 statement
of the same operation: uav_ppo_loss (separate and packed) and uav_ppo_loss_from_y at every action width / hidden size they
instantiate, uav_policy_sample(_at) + uav_store_transition, uav_gae, uav_adv_stats / uav_adv_normalise(_inline).  The cases, the
f64 statements and the near-branch rule are in tests/_ppo_sample_cases.py (checked on the CPU by test_ppo_sample_cases_host.py).

Two kinds of tolerance, no third:
  (a) a bound derived from the kernel's arithmetic, stated where it is used (bit equality is the tightest of them);
  (b) `check_b`: err_kernel <= 2 * err_torch_f32 + 2 f32 ulps of the compared scale, the yardstick being the SAME statement in
      f32 torch on the CPU.  Each (b) comparison prints its figures (pytest -s).  -m gpu."""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

import _ppo_sample_cases as pc
from _ppo_sample_cases import BETA, CLIP, CLIP_DYADIC, EPS, F32, F64, check_b, ulp32
from oracle import ppo_oracle as po
from oracle import procedural_oracle as pro

pytestmark = pytest.mark.gpu

DEV = "cuda:0"

# MEASURED on an MI355X: err_kernel / err_torch_f32 of every check_b comparison, the largest over the n (GAE: over T, n and
# done probability) of a row.  Where a ratio is above 2 the kernel's error is a few ulps that the 2-ulp floor carries (f32 torch
# happened to land closer): the comparison nearest its allowance 2 err_torch_f32 + floor uses 0.93 of it (GAE standard, n = 1,
# T = 64: 3.5e-6 against 9.5e-7 with a floor of 1.9e-6), the nearest of the loss 0.88 (ratio = 1, A = 4, n = 1: 1.9e-8 against
# 3.3e-9, floor 1.5e-8).  The three sums are f64 sums of f32 terms: their ratios are large where torch's f32 mean happened to
# cancel its errors (value sum, from_y H = 128, n = 257: 6.6e-7 against 2.8e-9), at a tenth of the floor or less.
#   uav_ppo_loss             A       2      3      4      5      6      8
#     sum surrogate               9.50   1.73   3.68   6.27   4.08   2.25
#     sum value                   1.46   3.51   1.00   1.00   1.01   1.15
#     sum entropy                 6.56   0.99   8.11   1.64   1.26   8.88
#     n dlogits                   1.49   3.20   2.14   2.12   2.00   2.14
#     n dvalue                    1.00   1.00   1.00   1.00   1.00   1.00
#     dhead_bias                  1.36   3.20   3.87   1.05   1.46   2.65
#     ratio = 1: n dlogits        0.82   0.90   5.74   0.74   1.00   1.07     (n dvalue 1.00 throughout)
#     value rows: n dlogits       1.51   1.00   2.20   1.80   0.43   2.70     (n dvalue 1.00; sums <= 2.5 but surrogate A = 2: 13.4)
#     closed clamp: n dlogits     1.00   1.00   1.00   1.00   1.00   1.00
#   uav_ppo_loss_from_y      H      64    128    256
#     sum surrogate               6.48  41.41  10.65
#     sum value                   5.69 238.48   5.81
#     sum entropy               139.58   1.35  40.84
#     dhead_bias                  2.89   1.28   4.17
#     n dlogits                   1.89   1.56   2.67      with bound (a) on top: at most 0.065 of the allowance used
#     n dvalue                    2.18   2.39   2.68      with bound (a) on top: at most 0.037 of the allowance used
#   uav_policy_sample probs: 1.00 at every width (the kernel's softmax has f32 torch's bits on these rows).
#   uav_gae                  reference_exact   standard   standard without last_val
#     gamma, lambda 0.99, 0.95       2.51          3.71          3.28
#     gamma, lambda 1, 1             2.21          1.90          1.82
#   uav_adv_normalise / uav_adv_normalise_inline: adv and ret 1.00 at every n.


@pytest.fixture(scope="module")
def ops():
    from uavppo import ops as o
    return o


def d(t):
    return t.to(DEV).contiguous()


def same(x, y):
    """bit for bit, NaN payloads included"""
    x, y = (torch.empty_like(t, memory_format=torch.contiguous_format).copy_(t).reshape(-1) for t in (x, y))
    return x.dtype == y.dtype and x.shape == y.shape and torch.equal(x.view(torch.uint8), y.view(torch.uint8))


# ----------------------------------------------------------------------------- uav_ppo_loss
def run_loss(ops, c, clip, beta=BETA, packed=False, fill=float("nan")):
    """-> (sums f64 [4], d total / d (logits | value) f32 [n, A + 1], dhead_bias f32 [A + 1]) on the CPU; the outputs start
    as `fill`, so an element the kernel does not write shows"""
    n, A = c["logits"].shape
    rest = [d(c[k]) for k in ("act", "logp_old", "adv", "ret", "val_old")]
    sums = torch.full((4,), fill, dtype=F64, device=DEV)
    db = torch.full((A + 1,), fill, device=DEV)
    if packed:
        dh = torch.full((n, A + 1), fill, device=DEV)
        ops.ppo_loss_heads(d(torch.cat([c["logits"], c["value"][:, None]], 1)), *rest, 1.0 / n, clip, beta, sums, dh, db)
        return sums.cpu(), dh.cpu(), db.cpu()
    dz, dv = torch.full((n, A), fill, device=DEV), torch.full((n,), fill, device=DEV)
    ops.ppo_loss(d(c["logits"]), d(c["value"]), *rest, 1.0 / n, clip, beta, loss_sums=sums, dlogits=dz, dvalue=dv, dhead_bias=db)
    return sums.cpu(), torch.cat([dz, dv[:, None]], 1).cpu(), db.cpu()


def check_ab(name, got, want, ref32, bound):
    """(b) with an input bound of kind (a) on top, element by element: err_kernel[i] <= 2 * err_torch_f32 + 2 ulps + bound[i].
    Prints the (b) ratio as check_b does and the largest share of its allowance an element uses."""
    err = (got.double() - want).abs()
    et = float((ref32.double() - want).abs().max())
    floor = 2 * ulp32(float(want.abs().max()))
    used = float((err / (2 * et + floor + bound)).max())
    ek = float(err.max())
    ratio = ek / et if et > 0 else float("inf") if ek > 0 else 0.0
    print(f"{name}: err_kernel {ek:.3e}  err_torch_f32 {et:.3e}  ratio {ratio:.2f}  floor {floor:.1e}"
          f"  largest bound (a) {float(bound.max()):.1e}  allowance used {used:.3f}")
    assert used <= 1, (name, used)
    return used


def compare_loss(tag, got, c, clip, what=("sums", "g", "dbias"), g_bound=None):
    """sums, n * gradients and dhead_bias against ppo_losses + autograd in f64, by (b); g_bound [n, A + 1]: a bound (a) on what
    the error of the case's inputs does to n * gradients, added to their allowance"""
    sums, g, db = got
    n, A = g.shape[0], g.shape[1] - 1
    r64, r32 = pc.loss_reference(c, F64, clip), pc.loss_reference(c, F32, clip)
    if "sums" in what:
        for k, (name, scale) in enumerate(zip(("surrogate", "value", "entropy"), pc.sum_scales(c, clip))):
            check_b(f"{tag} | sum {name}", sums[k:k + 1], r64["sums"][k:k + 1], r32["sums"][k:k + 1], scale=scale)
    if "g" in what and g_bound is not None:
        check_ab(f"{tag} | n dlogits", g[:, :A].double() * n, r64["g"][:, :A], r32["g"][:, :A], g_bound[:, :A])
        check_ab(f"{tag} | n dvalue", g[:, A].double() * n, r64["g"][:, A], r32["g"][:, A], g_bound[:, A])
    elif "g" in what:
        check_b(f"{tag} | n dlogits", g[:, :A].double() * n, r64["g"][:, :A], r32["g"][:, :A])
        check_b(f"{tag} | n dvalue", g[:, A].double() * n, r64["g"][:, A], r32["g"][:, A])
    if "dbias" in what:
        # a column's elements have either sign: the floor is taken at the largest column sum of magnitudes
        col = float((r64["g"] / n).abs().sum(0).max())
        check_b(f"{tag} | dhead_bias", db, r64["dbias"], r32["dbias"], scale=col)


@pytest.mark.parametrize("n", pc.LOSS_NS)
@pytest.mark.parametrize("A", pc.WIDTHS)
def test_ppo_loss_matches_f64(ops, A, n):
    """Every width the ABI instantiates, n = 1, around one block's 256 samples and 20 blocks: the three sums, every gradient
    element and dhead_bias by (b); no NaN counted; the packed form and a second call give the same bits."""
    c = pc.loss_case(n, A)
    assert c["altered"] <= pc.CAP * n
    got = run_loss(ops, c, CLIP)
    assert got[0][3] == 0
    compare_loss(f"ppo_loss A={A} n={n}", got, c, CLIP)
    for other in (run_loss(ops, c, CLIP, packed=True), run_loss(ops, c, CLIP, fill=-3e30)):
        for x, y in zip(got, other):
            assert same(x, y)


@pytest.mark.parametrize("A", pc.WIDTHS)
def test_ppo_loss_ratio_exactly_one(ops, A):
    """logp_old = what uav_policy_sample returns for the same logits and actions -- loss_core.h promises the loss kernel's own
    bits, so every ratio is expf(0) = 1, inside the clip.  (a): the surrogate sum is then -sum(adv), exact for advantages that
    are multiples of 1/8 (one ratio an ulp off 1 would show: its product with adv is off by 2^-24 |adv| or more).  The
    gradients by (b) against f64 with ITS own log-probability as logp_old: -inv_n A (onehot - q) plus the entropy term."""
    for n in (1, 257):
        c = pc.ratio_one_case(n, A, seed=n + A)
        _, lp, _, nan = ops.policy_sample(d(c["logits"]), forced_act=d(c["act"]))
        assert nan.item() == 0
        sums, g, db = run_loss(ops, dict(c, logp_old=lp.cpu()), CLIP)
        assert sums[3] == 0 and float(sums[0]) == -float(c["adv"].double().sum())
        tag = f"ppo_loss ratio=1 A={A} n={n}"
        r64 = pc.loss_reference(dict(c, logp_old=pc.own_logp(c, F64)), F64)
        r32 = pc.loss_reference(dict(c, logp_old=pc.own_logp(c, F32)), F32)
        check_b(f"{tag} | n dlogits", g[:, :A].double() * n, r64["g"][:, :A], r32["g"][:, :A])
        check_b(f"{tag} | n dvalue", g[:, A].double() * n, r64["g"][:, A], r32["g"][:, A])


@pytest.mark.parametrize("A", pc.WIDTHS)
def test_ppo_loss_value_branch_points(ops, A):
    """_ppo_sample_cases.VALUE_ROWS, dyadic numbers with clip = 0.25: V - v_old == +-clip is in range (gradient 2 (V - R)),
    |dv| > clip with e1 > e2, e1 < e2 and e1 == e2.  (a): gV is exact in f32 in every row, so dvalue is f32's
    (0.5 inv_n) gV bit for bit -- for the tie outside the clip that is 0.5 inv_n 0.5 (d1 + d2) with d2 = 0 -- and the value-loss
    sum is exact.  The host file ties VALUE_GV to f64 autograd."""
    c = pc.value_clip_case(A)
    n = len(pc.VALUE_ROWS)
    sums, g, db = run_loss(ops, c, CLIP_DYADIC)
    assert np.array_equal(g[:, A].numpy(), pc.value_clip_dvalue_f32(n)), (g[:, A].numpy(), pc.value_clip_dvalue_f32(n))
    t = pc.terms64(c["logits"].double(), c["value"].double(), c, CLIP_DYADIC)
    assert float(sums[1]) == float(0.5 * torch.max(t["e1"], t["e2"]).sum()) and sums[3] == 0
    compare_loss(f"ppo_loss value rows A={A}", (sums, g, db), c, CLIP_DYADIC)


@pytest.mark.parametrize("A", pc.WIDTHS)
def test_ppo_loss_closed_clamp_has_no_policy_gradient(ops, A):
    """Logits [60, 0, ..., -60] with the action on the clamped class at either end: (a) the policy gradient is exactly 0 -- the
    gradients are those of the same call without advantages -- and the entropy gradient remains, by (b)."""
    c = pc.clamp_case(A)
    got = run_loss(ops, c, CLIP)
    zero = run_loss(ops, dict(c, adv=torch.zeros(4)), CLIP)
    assert torch.equal(got[1], zero[1]) and got[0][3] == 0
    if A > 2:                                                # (two classes: p = (1, 0) in f32 and the entropy gradient is 0 too)
        assert (got[1][:, :A].abs().max(1).values > 0).all()
    compare_loss(f"ppo_loss closed clamp A={A}", got, c, CLIP, what=("g",))


@pytest.mark.parametrize("sign", [1, -1, 0])
@pytest.mark.parametrize("A", pc.WIDTHS)
def test_ppo_loss_overflowing_ratio(ops, A, sign):
    """logp_old = -200: the ratio is +inf in f32.  Loss sums and gradients are finite, +inf, -inf or NaN exactly where the f64
    statement, rounded to the f32 the kernel computes a sample in, is: A > 0 and A = 0 are clipped away -- a finite loss and (a)
    exactly the gradient of the same call without advantages, not 0 * inf = NaN; A < 0 keeps the unclipped side, whose loss
    and policy gradient are past f32's range: +inf and +-inf by the sign of (onehot - q)."""
    c = pc.overflow_case(A, sign)
    n = c["logits"].shape[0]
    sums, g, _ = run_loss(ops, c, CLIP)
    r64 = pc.loss_reference(c, F64)
    with np.errstate(over="ignore"):
        want_s, want_g = (r64["sums"] / n).float(), (r64["g"] / n).float()
    assert sums[3] == 0
    for got, want in ((sums[:3].float(), want_s), (g, want_g)):
        for mask in (torch.isnan, torch.isposinf, torch.isneginf):
            assert torch.equal(mask(got), mask(want)), (mask.__name__, got, want)
    if sign >= 0:
        own = dict(c, adv=torch.zeros(n), logp_old=pc.own_logp(c, F32))
        assert torch.equal(g, run_loss(ops, own, CLIP)[1])
    else:
        assert torch.isinf(g[:, :A]).all() and torch.isfinite(g[:, A]).all() and sums[0] == float("inf")


@pytest.mark.parametrize("A", pc.WIDTHS)
def test_ppo_loss_nan_logit_is_counted_once(ops, A):
    """A row with a NaN logit -- one or several -- counts once in sums[3]; every other row keeps the bits of a clean call."""
    n = 300
    c = pc.loss_case(n, A, seed=3 + A)
    clean = run_loss(ops, c, CLIP)
    assert clean[0][3] == 0
    for row, cols in ((17, [A - 1]), (0, [0, A - 1]), (n - 1, list(range(A)))):
        z = c["logits"].clone()
        z[row, cols] = float("nan")
        sums, g, _ = run_loss(ops, dict(c, logits=z), CLIP)
        assert sums[3] == 1
        keep = [r for r in range(n) if r != row]
        assert same(g[keep], clean[1][keep]) and torch.isnan(g[row, :A]).all()


def test_ppo_loss_refuses_seven_actions(ops):
    c = pc.loss_case(4, 7, seed=1)
    outs = [torch.full((4,), 7.0, dtype=F64, device=DEV), torch.full((4, 7), 7.0, device=DEV), torch.full((4,), 7.0, device=DEV),
            torch.full((8,), 7.0, device=DEV)]
    rest = [d(c[k]) for k in ("act", "logp_old", "adv", "ret", "val_old")]
    with pytest.raises(RuntimeError, match=r"uav_ppo_loss failed \([1-9]\d*\).*n_act=7"):
        ops.ppo_loss(d(c["logits"]), d(c["value"]), *rest, 0.25, CLIP, BETA, loss_sums=outs[0], dlogits=outs[1], dvalue=outs[2],
                     dhead_bias=outs[3])
    torch.cuda.synchronize()
    for o in outs:
        assert (o == 7.0).all()
    with pytest.raises(RuntimeError, match="n_act=7"):
        ops.policy_sample(d(c["logits"]))


# ----------------------------------------------------------------------------- uav_ppo_loss_from_y
@pytest.mark.parametrize("n,H", [(n, H) for H in pc.FROM_Y_HS for n in pc.FROM_Y_NS] + [pc.FROM_Y_BIG])
def test_ppo_loss_from_y_matches_f64(ops, n, H):
    """heads = y W^T + b in f64, then the loss; the yardstick is the same in f32 torch.  The sums and dhead_bias by (b).
    n * dheads needs more than (b)'s factor 2 at some shapes (up to 2.7 at H = 256, n = 255: the MFMA accumulation order
    against torch's dot product, a few ulps of a head either way), so its elements get a bound (a) on top: the heads' own
    rounding error, _ppo_sample_cases.heads_error_bound, propagated through the loss by from_y_gradient_bound.
    y has exactly n rows, so a row past the end that reached a sum or a gradient shows (the kernel loads whole 16-row
    tiles); a second call gives the same bits."""
    c = pc.from_y_case(n, H)
    assert c["altered"] <= pc.CAP * n
    outs = []
    for fill in (float("nan"), -3e30):
        sums = torch.full((4,), fill, dtype=F64, device=DEV)
        dh, db = torch.full((n, 6), fill, device=DEV), torch.full((6,), fill, device=DEV)
        ops.ppo_loss_from_y(d(c["y"]), d(c["w"]), d(c["b"]), *[d(c[k]) for k in ("act", "logp_old", "adv", "ret", "val_old")],
                            1.0 / n, CLIP, BETA, sums, dh, db)
        outs.append((sums.cpu(), dh.cpu(), db.cpu()))
    for x, y in zip(*outs):
        assert same(x, y)
    assert outs[0][0][3] == 0
    compare_loss(f"ppo_loss_from_y H={H} n={n}", outs[0], c, CLIP, g_bound=pc.from_y_gradient_bound(c))


# ----------------------------------------------------------------------------- uav_policy_sample
def check_draws(ops, tag, logits, u):
    """Every row's action is the inverse CDF restated in f32 numpy from the kernel's own probs -- exactly, no row skipped;
    probs against the f64 softmax by (b); (a) logp is logf of the restated argument q[a] = p[a] / psum clamped to
    [eps, 1 - eps], within 2 ulps of the f64 logarithm of that argument."""
    act, logp, probs, nan = ops.policy_sample(d(logits), u=d(u), want_probs=True)
    assert nan.item() == 0
    P, a = probs.cpu().numpy(), act.cpu().numpy()
    assert np.array_equal(a, pc.inverse_cdf_f32(P, u.numpy()))
    check_b(f"{tag} | probs", probs.cpu(), torch.softmax(logits.double(), -1), torch.softmax(logits, -1))
    want = np.log(pc.logp_argument_f32(P, a).astype(np.float64))
    err = np.abs(logp.cpu().numpy().astype(np.float64) - want)
    assert (err <= 2 * np.spacing(np.abs(want).astype(np.float32))).all(), (err / np.spacing(np.abs(want).astype(np.float32))).max()
    return a


@pytest.mark.parametrize("A", pc.WIDTHS)
def test_policy_sample_injected_uniforms(ops, A):
    logits, u = pc.sample_rows(1000, A, seed=A)
    a = check_draws(ops, f"policy_sample A={A}", logits, u)
    assert len(np.unique(a)) == A


@pytest.mark.parametrize("A", pc.WIDTHS)
def test_policy_sample_planted_uniforms(ops, A):
    """u = 0 with a first class of probability 0 skips it, u = nextafter(1, 0), a last class of probability 0, equal logits:
    _ppo_sample_cases.planted_sample_rows; where the row decides the action by itself it is the expected one."""
    z, u, want = pc.planted_sample_rows(A)
    a = check_draws(ops, f"policy_sample planted A={A}", z, u)
    known = want >= 0
    assert np.array_equal(a[known], want[known]), (a, want)


@pytest.mark.parametrize("A", pc.WIDTHS)
def test_policy_sample_all_minus_inf_row_counts_one_nan(ops, A):
    logits, u = pc.sample_rows(300, A, seed=7)
    clean = ops.policy_sample(d(logits), u=d(u))
    z = logits.clone()
    z[257] = float("-inf")
    act, logp, _, nan = ops.policy_sample(d(z), u=d(u))
    assert nan.item() == 1 and clean[3].item() == 0
    keep = [r for r in range(300) if r != 257]
    assert torch.equal(act[keep], clean[0][keep]) and same(logp[keep], clean[1][keep])


@pytest.mark.parametrize("iteration", [0, 3])
@pytest.mark.parametrize("index_offset", [0, 1000])
@pytest.mark.parametrize("n", [255, 256, 257])
@pytest.mark.parametrize("A", [5, 8])
def test_policy_sample_counter_rng(ops, A, n, index_offset, iteration):
    """Row i draws with action_uniform(seed, counter, index_offset + i, iteration): the action is the oracle's inverse CDF at
    that uniform over the kernel's own probs, every row."""
    seed, counter = 0x1234ABCD5678, 7
    logits, _ = pc.sample_rows(n, A, seed=n + A)
    act, _, probs, nan = ops.policy_sample(d(logits), seed=seed, counter=counter, want_probs=True, index_offset=index_offset,
                                           iteration=iteration)
    u = pro.action_uniform(seed, counter, index_offset + np.arange(n), iteration)
    assert u.dtype == np.float32 and nan.item() == 0
    assert np.array_equal(act.cpu().numpy(), pro.sample_inverse_cdf(probs.cpu().numpy(), u))
    assert np.array_equal(act.cpu().numpy(), pc.inverse_cdf_f32(probs.cpu().numpy(), u))


# ----------------------------------------------------------------------------- uav_policy_sample_at + uav_store_transition
SENT_I, SENT_F, SENT_U8 = -77, -123.25, 0xAB


@pytest.mark.parametrize("t", [0, 2, 4])
@pytest.mark.parametrize("A", [5, 3])
@pytest.mark.parametrize("N", [1, 257])
def test_policy_sample_at_and_store_transition_write_column_t_only(ops, N, A, t):
    T = 5
    g = torch.Generator().manual_seed(N + A + t)
    heads = d(2.0 * torch.randn(N, T, A + 1, generator=g))
    act_out = torch.full((N,), SENT_I, dtype=torch.int32, device=DEV)
    act_buf = torch.full((N, T), SENT_I, dtype=torch.int32, device=DEV)
    val_buf, logp_buf = torch.full((N, T), SENT_F, device=DEV), torch.full((N, T), SENT_F, device=DEV)
    nan = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.policy_sample_at(heads, t, act_out, act_buf, val_buf, logp_buf, nan, seed=99, iteration=2, index_offset=1000)
    act, logp, _, nan2 = ops.policy_sample(heads[:, t, :A].contiguous(), seed=99, counter=t, iteration=2, index_offset=1000)
    assert nan.item() == 0 and nan2.item() == 0
    assert torch.equal(act_out, act) and torch.equal(act_buf[:, t], act)
    assert same(logp_buf[:, t].contiguous(), logp) and same(val_buf[:, t].contiguous(), heads[:, t, A].contiguous())
    others = [k for k in range(T) if k != t]
    assert (act_buf[:, others] == SENT_I).all() and (val_buf[:, others] == SENT_F).all() and (logp_buf[:, others] == SENT_F).all()

    keep0 = (torch.rand(N, generator=g) < 0.7).float()
    rew, done = torch.randn(N, generator=g), (torch.rand(N, generator=g) < 0.3).float()
    flags = torch.randint(0, 4, (N,), generator=g, dtype=torch.uint8)
    keep = d(keep0)
    bufs = [torch.full((N, T), SENT_F, device=DEV) for _ in range(3)] + [torch.full((N, T), SENT_U8, dtype=torch.uint8, device=DEV)]
    ops.store_transition(t, keep, d(rew), d(done), d(flags), *bufs)
    for buf, src in zip(bufs, (keep0, rew, done, flags)):
        assert same(buf[:, t].contiguous().cpu(), src)
    for buf, sent in zip(bufs, (SENT_F, SENT_F, SENT_F, SENT_U8)):
        assert (buf[:, others] == sent).all()
    assert torch.equal(keep.cpu(), 1.0 - done)


def test_policy_sample_at_and_store_transition_refusals(ops):
    from uavppo import _lib
    N, T, A = 4, 5, 5
    heads = d(torch.randn(N, T, A + 1))
    act_out = torch.full((N,), SENT_I, dtype=torch.int32, device=DEV)
    act_buf = torch.full((N, T), SENT_I, dtype=torch.int32, device=DEV)
    val_buf, logp_buf = torch.full((N, T), SENT_F, device=DEV), torch.full((N, T), SENT_F, device=DEV)
    nan = torch.zeros(1, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match=r"uav_policy_sample_at failed \([1-9]\d*\).*T=5 t=5"):
        ops.policy_sample_at(heads, T, act_out, act_buf, val_buf, logp_buf, nan)
    for stride in (A, A - 1):                                # the value is read at column n_act: the row must hold it
        rc = _lib.lib().uav_policy_sample_at(ops._h(heads), ops._p(heads), stride, N, A, 0, 0, 0, None, ops._p(act_out), T, 0,
                                             ops._p(act_buf), ops._p(val_buf), ops._p(logp_buf), ops._p(nan), ops._stream())
        assert rc != 0 and f"heads_stride={stride}" in _lib.lib().uav_last_error().decode()
    bufs = [torch.full((N, T), SENT_F, device=DEV) for _ in range(3)] + [torch.full((N, T), SENT_U8, dtype=torch.uint8, device=DEV)]
    keep = torch.ones(N, device=DEV)
    with pytest.raises(RuntimeError, match=r"uav_store_transition failed \([1-9]\d*\).*T=5 t=5"):
        ops.store_transition(T, keep, torch.zeros(N, device=DEV), torch.ones(N, device=DEV),
                             torch.zeros(N, dtype=torch.uint8, device=DEV), *bufs)
    torch.cuda.synchronize()
    assert (act_out == SENT_I).all() and (act_buf == SENT_I).all() and (val_buf == SENT_F).all() and (logp_buf == SENT_F).all()
    assert all((b == s).all() for b, s in zip(bufs, (SENT_F, SENT_F, SENT_F, SENT_U8))) and (keep == 1).all()


# ----------------------------------------------------------------------------- uav_gae
@pytest.mark.parametrize("gamma,lam", pc.GAE_COEFS)
@pytest.mark.parametrize("mode", ["reference_exact", "standard", "standard_no_last_val"])
def test_gae_matches_f64_loop(ops, mode, gamma, lam):
    """Each mode's recurrence as an f64 loop; the yardstick of (b) is the oracle's sequential f32 loop (the wave scan
    re-associates it).  T around the scan's 64-step chunk, n around a block's 4 rows, done never / sometimes / always.  Without
    last_val the standard mode bootstraps from 0: the bits of a call with an explicit zero vector."""
    worst = 0.0
    for T in pc.GAE_TS:
        for n in pc.GAE_NS:
            for p_done in pc.GAE_P_DONE:
                rew, val, done, last = pc.gae_case(n, T, p_done, seed=1000 * n + T)
                dr, dv, dd = (d(torch.from_numpy(x)) for x in (rew, val, done))
                if mode == "reference_exact":
                    want = pc.gae_f64(rew, val, done, None, gamma, lam, mode)
                    ref32 = po.gae_reference_exact(rew, val, done, gamma, lam)
                    got = ops.gae(dr, dv, dd, gamma, lam, mode)
                elif mode == "standard":
                    want = pc.gae_f64(rew, val, done, last, gamma, lam, mode)
                    ref32 = po.gae_standard(rew, val, done, last, gamma, lam)
                    got = ops.gae(dr, dv, dd, gamma, lam, mode, last_val=d(torch.from_numpy(last)))
                else:
                    zero = np.zeros(n, np.float32)
                    want = pc.gae_f64(rew, val, done, None, gamma, lam, "standard")
                    ref32 = po.gae_standard(rew, val, done, zero, gamma, lam)
                    got = ops.gae(dr, dv, dd, gamma, lam, "standard")
                    assert same(got, ops.gae(dr, dv, dd, gamma, lam, "standard", last_val=d(torch.from_numpy(zero))))
                worst = max(worst, check_b(f"gae {mode} gamma={gamma} | n={n} T={T} p_done={p_done}", got.cpu(),
                                           torch.from_numpy(want), torch.from_numpy(ref32)))
    print(f"gae {mode} gamma={gamma}: worst ratio {worst:.2f}")


# ----------------------------------------------------------------------------- uav_adv_stats / uav_adv_normalise(_inline)
@pytest.mark.parametrize("n", pc.ADV_NS)
def test_adv_stats_and_normalise_match_f64(ops, n):
    """(a) the statistics are f64 sums of exactly converted f32 values: both within 1e-12 of the f64 sums, the count exact; the
    normalised advantages and the returns of both forms by (b) against the formula in f64."""
    adv, val = pc.adv_case(n)
    a, v = d(adv), d(val)
    stats = ops.adv_stats(a)
    assert same(stats, ops.adv_stats(a))
    s = stats.cpu().numpy()
    s0, s1 = float(adv.double().sum()), float((adv.double() ** 2).sum())
    assert s[2] == n and abs(s[0] - s0) <= 1e-12 * abs(s0) and abs(s[1] - s1) <= 1e-12 * s1, (s, s0, s1)
    for inline in (False, True):
        ga, gr = (ops.adv_normalise_inline if inline else ops.adv_normalise)(a, v, stats)
        a64, r64 = pc.normalise_f64(adv, val, inline)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            a32, r32 = pc.normalise_f32(adv, val, inline)
        tag = f"adv_normalise{'_inline' if inline else ''} n={n}"
        if inline and n == 1:
            assert torch.isnan(ga).all() and torch.isfinite(gr).all() and gr.item() == (adv + val).item()
            continue
        check_b(f"{tag} | adv", ga.cpu(), a64, a32)
        check_b(f"{tag} | ret", gr.cpu(), r64, r32)


@pytest.mark.parametrize("n", pc.ADV_NS)
def test_adv_stats_of_integers_are_exact(ops, n):
    """Small integers: every partial sum is an integer far below 2^53, so both sums are exact in any order and one dropped or
    doubled element anywhere shows, also past the 512-block cap."""
    x = torch.randint(-8, 9, (n,), generator=torch.Generator().manual_seed(n)).float()
    s = ops.adv_stats(d(x)).cpu()
    assert s[0] == x.double().sum() and s[1] == (x.double() ** 2).sum() and s[2] == n


@pytest.mark.parametrize("n", [2, 1025, 2097152 + 513])
def test_adv_normalise_constant_buffer_guard(ops, n):
    """std < 1e-6 divides by 1 + 1e-6 (train_ppo2.0.py:37-39): a constant buffer normalises to 0 and the returns are V."""
    a, v = torch.full((n,), 0.25, device=DEV), d(torch.randn(n, generator=torch.Generator().manual_seed(n)))
    ga, gr = ops.adv_normalise(a, v, ops.adv_stats(a))
    assert (ga == 0).all() and torch.equal(gr, v)
