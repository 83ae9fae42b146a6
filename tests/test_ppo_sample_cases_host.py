"""tests/_ppo_sample_cases.py on the CPU: the builders keep their cap for every seed and shape tests/test_gpu_loss_kernels.py uses,
every planted sample sits where it is meant to in f64, and f32 torch -- the yardstick of tolerance (b) -- meets the f64 statement
on the built cases."""
import numpy as np
import pytest
import torch

import _ppo_sample_cases as pc
from _ppo_sample_cases import CLIP, CLIP_DYADIC, EPS, F32, F64

# The f64 statement is some 40 f32 operations a sample when run in f32, each within 2^-24 of its result, and the ratio's exp
# turns the absolute error of logp - logp_old (|logp| <= 16) into a relative one: 2e-5 of the compared scale bounds all of it
# with room, and a yardstick that lost a term or took another branch misses it by orders of magnitude.
SANE = 2e-5

RANDOM_CASES = [("loss", n, A) for A in pc.WIDTHS for n in pc.LOSS_NS] \
    + [("from_y", n, H) for H in pc.FROM_Y_HS for n in pc.FROM_Y_NS] + [("from_y",) + pc.FROM_Y_BIG]


def _z_v(c):
    if "y" in c:
        heads = pc.heads_of(c, F64)
        return heads[:, :-1], heads[:, -1]
    return c["logits"].double(), c["value"].double()


def _sane(c, clip=CLIP):
    r64, r32 = pc.loss_reference(c, F64, clip), pc.loss_reference(c, F32, clip)
    for k, scale in zip(range(3), pc.sum_scales(c, clip)):
        assert abs(float(r32["sums"][k] - r64["sums"][k])) <= SANE * max(scale, 1e-30), (k, r32["sums"][k], r64["sums"][k])
    assert float((r32["g"] - r64["g"]).abs().max()) <= SANE * float(r64["g"].abs().max())
    col = (r64["g"] / r64["g"].shape[0]).abs().sum(0).max()
    assert float((r32["dbias"].double() - r64["dbias"]).abs().max()) <= SANE * float(col)
    return r64


@pytest.mark.parametrize("kind,n,w", RANDOM_CASES)
def test_random_cases_keep_the_cap_and_f32_torch_meets_f64(kind, n, w):
    c = pc.loss_case(n, w) if kind == "loss" else pc.from_y_case(n, w)
    assert c["altered"] <= pc.CAP * n, (kind, n, w, c["altered"])
    z64, v64 = _z_v(c)
    near_r, near_v = pc.near_branch(z64, v64, c, CLIP)
    # what is left next to a ratio edge has no advantage; nothing is left next to a value branch point
    assert (c["adv"][near_r] == 0).all() and not near_v.any()
    t = pc.terms64(z64, v64, c, CLIP)
    if n >= 255:                                             # the branches are all populated
        r, dv = t["ratio"], t["dv"]
        assert (r < 1 - CLIP).sum() > n // 20 and (r > 1 + CLIP).sum() > n // 20 and ((r - 1).abs() < CLIP).sum() > n // 4
        assert (dv.abs() > CLIP).sum() > n // 4 and (dv.abs() < CLIP).sum() > n // 4
        out = dv.abs() > CLIP
        assert (out & (t["e1"] > t["e2"])).sum() > n // 20 and (out & (t["e1"] < t["e2"])).sum() > n // 20
    _sane(c)
    if kind == "from_y":
        # bound (a) on the heads holds for f32 torch's product too, and what it does to n * dheads stays far below a gradient
        dh = pc.heads_error_bound(c)
        assert ((pc.heads_of(c, F32).double() - pc.heads_of(c, F64)).abs() <= dh).all()
        gb = pc.from_y_gradient_bound(c)
        assert torch.isfinite(gb).all() and (gb >= 0).all() and float(gb.max()) < 1e-2


@pytest.mark.parametrize("A", pc.WIDTHS)
def test_ratio_one_case(A):
    for n in (1, 257):
        c = pc.ratio_one_case(n, A, seed=n + A)
        for dtype in (F64, F32):                             # each arithmetic with its own log-probability: ratio == 1 exactly
            cc = dict(c, logp_old=pc.own_logp(c, dtype))
            lp = pc.own_logp(cc, dtype)
            assert torch.equal((lp - cc["logp_old"]).exp(), torch.ones(n, dtype=dtype))
        c64 = dict(c, logp_old=pc.own_logp(c, F64))          # (kept in f64: loss_reference's .to(dtype) leaves it alone)
        r64 = pc.loss_reference(c64, F64)
        assert float(r64["sums"][0]) == -float(c["adv"].double().sum())         # surrogate = adv, exactly
        # the gradient is -inv_n A (onehot - q) plus the entropy term: with no entropy coefficient only the first is left
        g0 = pc.loss_reference(c64, F64, beta=0.0)["g"][:, :A]
        t = pc.terms64(c["logits"].double(), c["value"].double(), c64, CLIP)
        q, open_ = t["q"], ((t["qa"] >= EPS) & (t["qa"] <= 1 - EPS)).double()
        onehot = torch.nn.functional.one_hot(c["act"].long(), A).double()
        assert torch.allclose(g0, -(open_ * c["adv"].double())[:, None] * (onehot - q), rtol=1e-12, atol=1e-14)


@pytest.mark.parametrize("A", pc.WIDTHS)
def test_value_clip_case(A):
    c = pc.value_clip_case(A)
    n = len(pc.VALUE_ROWS)
    t = pc.terms64(c["logits"].double(), c["value"].double(), c, CLIP_DYADIC)
    dv, e1, e2 = t["dv"], t["e1"], t["e2"]
    assert dv[0] == CLIP_DYADIC and dv[1] == -CLIP_DYADIC and e1[0] == e2[0] and e1[1] == e2[1]
    assert dv[2] > CLIP_DYADIC and e1[2] > e2[2] and dv[3] > CLIP_DYADIC and e1[3] < e2[3] and dv[4] > CLIP_DYADIC and e1[4] == e2[4]
    assert dv[5] < -CLIP_DYADIC and e1[5] > e2[5] and dv[6] < -CLIP_DYADIC and e1[6] < e2[6] and dv[7] < -CLIP_DYADIC and e1[7] == e2[7]
    assert dv[8] == 0 and 0 < dv[9] < CLIP_DYADIC
    r64 = pc.loss_reference(c, F64, CLIP_DYADIC)
    # f64 autograd: n * d total / dV = 0.5 gV up to the rounding of 1 / n; torch splits a tie of max 1/2 - 1/2 as the kernel does
    assert torch.allclose(r64["g"][:, A], 0.5 * torch.tensor(pc.VALUE_GV, dtype=F64), rtol=1e-15, atol=0)
    assert float(r64["sums"][1]) == float(0.5 * torch.max(e1, e2).sum())
    assert pc.value_clip_dvalue_f32(n).dtype == np.float32
    _sane(c, CLIP_DYADIC)


@pytest.mark.parametrize("A", pc.WIDTHS)
def test_clamp_case(A):
    c = pc.clamp_case(A)
    t = pc.terms64(c["logits"].double(), c["value"].double(), c, CLIP)
    assert (t["qa"][[0, 2]] > 1 - EPS).all() and (t["qa"][[1, 3]] < EPS).all()
    r64 = pc.loss_reference(c, F64)
    rz = pc.loss_reference(dict(c, adv=torch.zeros(4)), F64)
    assert torch.equal(r64["g"], rz["g"])                    # no policy gradient ...
    assert (r64["g"][:, :A].abs().max(1).values > 0).all()   # ... and the entropy gradient remains
    _sane(c)


@pytest.mark.parametrize("A", pc.WIDTHS)
def test_overflow_case(A):
    for sign in (1, -1, 0):
        c = pc.overflow_case(A, sign)
        t = pc.terms64(c["logits"].double(), c["value"].double(), c, CLIP)
        big = float(np.finfo(np.float32).max)
        assert (t["ratio"] > big).all() and torch.isfinite(t["ratio"]).all()      # past f32, finite in f64
        with np.errstate(over="ignore"):
            assert np.isinf(np.exp((t["logp"].float() - c["logp_old"]).numpy())).all()
        r64 = pc.loss_reference(c, F64)
        assert torch.isfinite(r64["g"]).all() and torch.isfinite(r64["sums"]).all()
        if sign >= 0:                                        # clipped away (or no advantage): no policy term at all
            r0 = pc.loss_reference(dict(c, adv=torch.zeros_like(c["adv"])), F64)
            assert torch.equal(r64["g"], r0["g"])
        else:                                                # the unclipped side is the minimum: a gradient no f32 holds
            assert (r64["g"][:, :A].abs() > big).all()


@pytest.mark.parametrize("A", pc.WIDTHS)
def test_sampling_restatement_and_planted_rows(A):
    # on exact f32 probabilities the restatement is oracle.procedural_oracle.sample_inverse_cdf
    from oracle import procedural_oracle as pro
    logits, u = pc.sample_rows(1000, A, seed=A)
    probs = torch.softmax(logits, -1).numpy()
    assert np.array_equal(pc.inverse_cdf_f32(probs, u.numpy()), pro.sample_inverse_cdf(probs, u.numpy()))
    z, pu, want = pc.planted_sample_rows(A)
    p = torch.softmax(z, -1).numpy()
    got = pc.inverse_cdf_f32(p, pu.numpy())
    known = want >= 0
    assert np.array_equal(got[known], want[known]), (got, want)
    assert pc.U_LAST < 1 and np.float32(pc.U_LAST) == np.float32(1) - np.float32(2.0 ** -24)
    assert (p[np.arange(len(got)), got][known] > 0).all()    # no decided row draws a class of probability 0
    qa = pc.logp_argument_f32(p, got)
    assert qa.dtype == np.float32 and (qa >= np.float32(EPS)).all() and (qa <= 1 - np.float32(EPS)).all()


def test_gae_f64_loops_meet_the_f32_oracle():
    from oracle import ppo_oracle as po
    for n, T, p in ((4, 65, 0.1), (5, 300, 0.0), (1, 1, 1.0), (9, 129, 1.0)):
        rew, val, done, last = pc.gae_case(n, T, p, seed=T)
        for gamma, lam in pc.GAE_COEFS:
            a = pc.gae_f64(rew, val, done, None, gamma, lam, "reference_exact")
            assert np.allclose(a, po.gae_reference_exact(rew, val, done, gamma, lam), rtol=1e-5, atol=1e-5 * np.abs(a).max())
            b = pc.gae_f64(rew, val, done, last, gamma, lam, "standard")
            assert np.allclose(b, po.gae_standard(rew, val, done, last, gamma, lam), rtol=1e-5, atol=1e-5 * np.abs(b).max())
            z = pc.gae_f64(rew, val, done, None, gamma, lam, "standard")
            assert np.array_equal(z, pc.gae_f64(rew, val, done, np.zeros(n, np.float32), gamma, lam, "standard"))
        if p == 1.0:                                         # every step ends an episode: the advantage is the step's delta
            assert np.array_equal(pc.gae_f64(rew, val, done, last, 0.99, 0.95, "standard"), rew.astype(np.float64) - val)


@pytest.mark.parametrize("n", pc.ADV_NS[:4])
def test_normalise_statements_agree(n):
    import warnings
    adv, val = pc.adv_case(n)
    for inline in (False, True):
        a64, r64 = pc.normalise_f64(adv, val, inline)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            a32, r32 = pc.normalise_f32(adv, val, inline)
        if n == 1 and inline:
            assert torch.isnan(a64).all() and torch.isnan(a32).all() and torch.isfinite(r64).all()
            continue
        assert torch.allclose(a32.double(), a64, rtol=1e-5, atol=1e-5) and torch.allclose(r32.double(), r64, rtol=1e-5, atol=1e-5)
