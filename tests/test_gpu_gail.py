"""GAIL on the GPU: the fused discriminator kernels (uav_disc_grad, uav_disc_reward; csrc/disc.hip) through uavppo.ops, GAILTrainer,
generate_expert_data and the train_ppo_gail script.  -m gpu.

The checker is built here from torch-CPU modules: nn.Sequential(Linear, ReLU, Linear, Sigmoid) -- the reference's discriminator is
exactly these four layers -- nn.BCELoss, optim.Adam, in float64 (the oracle) and float32 (the yardstick of what f32 can do).

Which f64 value is "the oracle" where the sigmoid saturates.  nn.BCELoss(nn.Sigmoid(z)) is evaluated by torch as
-max(log(1 - D), -100) with D already ROUNDED: for a label-0 row D becomes exactly 1 beyond z = 36.74 in float64 (16.6 in
float32), so the loss term jumps from z to 100 there, and the backward pass, (D - y) / max(D (1 - D), 1e-12) * D (1 - D), returns 0
instead of D - y (it starts to shrink at z = 27.6).  Both are rounding artefacts of composing the two layers, not properties of
the loss; the kernel's contract (include/uavppo.h) is the exact value: loss min(softplus(-+z), 100), gradient D - y through the
logit -- the issue's "f64 BCEWithLogits gradient".  So the oracle takes the logit from the first three layers of the f64 module and
evaluates F.binary_cross_entropy_with_logits on it (per-row terms clamped at 100 for the loss figures, as nn.BCELoss clamps), and
`test_oracle_forms_agree_where_nothing_saturates` pins that form to the literal nn.BCELoss(nn.Sigmoid) module, loss and gradient,
at nn.Linear's default scale, where no row comes near saturation.  At 30 x that scale |z| reaches several hundred and the
literal f64 module is off by tens of percent in both; the f32 yardstick uses the same logit form in float32.

Tolerance (the project's rule, tests/test_gpu_lstm.py): per tensor, relative L2 error against the f64 oracle <= 2 * e_f32 + 2e-7,
e_f32 = the error of torch-CPU f32 autograd against the same oracle on the same inputs; the factor 2 covers a different but equally
valid summation order, the floor is one f32 ulp of headroom.  Loss sums: 1e-6 relative."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import ppo_oracle as po

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "uav-wrf-les-ppo-lstm_amd")
H = 128
KEYS = ("0.weight", "0.bias", "2.weight", "2.bias")
PARITY = {}


@pytest.fixture(scope="module")
def ops():
    from uavppo import ops as o
    return o


@pytest.fixture(scope="module", autouse=True)
def _write_parity():
    yield
    out_dir = os.environ.get("UAVPPO_PARITY_DIR")          # where to keep the measured errors (profiles/gail_parity.json came from it)
    if PARITY and out_dir and os.path.isdir(out_dir):
        with open(os.path.join(out_dir, "gail_parity.json"), "w") as f:
            json.dump(PARITY, f, indent=1, sort_keys=True)


def dev(x, dtype=None):
    t = torch.as_tensor(x)
    return (t if dtype is None else t.to(dtype)).to(DEV).contiguous()


# ------------------------------------------------------------------------------------------------ the checker
def checker(flat, od, na, dtype):
    """The reference's network as a torch-CPU module in `dtype`, loaded from a flat parameter vector in state_dict order."""
    net = nn.Sequential(nn.Linear(od + na, H), nn.ReLU(), nn.Linear(H, 1), nn.Sigmoid()).to(dtype)
    sd, o = {}, 0
    for k, v in net.state_dict().items():
        sd[k] = torch.as_tensor(flat[o:o + v.numel()]).detach().cpu().to(dtype).reshape(v.shape)
        o += v.numel()
    assert o == len(flat)
    net.load_state_dict(sd)
    return net


def default_flat(od, na, seed, scale=1.0):
    """nn.Linear's default initialisation (times `scale`), flat f32."""
    torch.manual_seed(seed)
    net = nn.Sequential(nn.Linear(od + na, H), nn.ReLU(), nn.Linear(H, 1), nn.Sigmoid())
    return torch.cat([v.reshape(-1) for v in net.state_dict().values()]).float() * scale


def sa_rows(obs, act, na, dtype):
    a = torch.as_tensor(act).long()
    hot = (a[:, None] == torch.arange(na)[None, :]).to(dtype)          # an action outside [0, na) sets no column
    return torch.cat([torch.as_tensor(obs).to(dtype), hot], 1)


def oracle(flat, obs_e, act_e, obs_p, act_p, na, dtype=torch.float64, inv_ne=None, inv_np=None, chunk=65536):
    """Losses and gradient of inv_ne * sum_e BCE(z, 1) + inv_np * sum_p BCE(z, 0) in `dtype` (see the module docstring):
    {'grad': flat, 'loss': [expert sum, policy sum] with nn.BCELoss's clamp at 100 per row, 'correct', 'z'}."""
    od = (obs_p if len(obs_p) else obs_e).shape[1]
    net = checker(flat, od, na, dtype)
    ne, npol = len(act_e), len(act_p)
    inv_ne = (1.0 / ne if ne else 0.0) if inv_ne is None else inv_ne
    inv_np = (1.0 / npol if npol else 0.0) if inv_np is None else inv_np
    sa = torch.cat([sa_rows(obs_e, act_e, na, dtype).reshape(ne, od + na), sa_rows(obs_p, act_p, na, dtype).reshape(npol, od + na)])
    y = torch.cat([torch.ones(ne, dtype=dtype), torch.zeros(npol, dtype=dtype)])
    w = torch.cat([torch.full((ne,), inv_ne, dtype=dtype), torch.full((npol,), inv_np, dtype=dtype)])
    loss, zs, correct = [0.0, 0.0], [], 0
    for s in range(0, ne + npol, chunk):
        sl = slice(s, s + chunk)
        z = net[:3](sa[sl]).squeeze(1)                                   # the logit: everything in front of the Sigmoid layer
        per = F.binary_cross_entropy_with_logits(z, y[sl], reduction="none")
        (per * w[sl]).sum().backward()                                   # gradients accumulate over the chunks
        cl = per.detach().clamp(max=100.0).double()
        lab = y[sl] > 0.5
        loss[0] += float(cl[lab].sum())
        loss[1] += float(cl[~lab].sum())
        zd = z.detach()
        correct += int(((zd > 0) & lab).sum() + ((zd < 0) & ~lab).sum())
        zs.append(zd)
    grad = torch.cat([p.grad.reshape(-1) for p in net.parameters()])
    return {"grad": grad, "loss": loss, "correct": correct, "z": torch.cat(zs)}


def tensors(flat, od, na):
    sizes = [H * (od + na), H, H, 1]
    return dict(zip(KEYS, torch.split(torch.as_tensor(flat).detach().cpu().double(), sizes)))


def rel_l2(a, ref):
    return float((a - ref).norm() / ref.norm().clamp(min=1e-300))


def check_grad(got, o64, o32, od, na, label):
    """The rule of the module docstring, per tensor; returns the measured errors."""
    g, r, f = tensors(got, od, na), tensors(o64["grad"], od, na), tensors(o32["grad"], od, na)
    out = {}
    for k in KEYS:
        e_got, e_f32 = rel_l2(g[k], r[k]), rel_l2(f[k], r[k])
        out[k] = {"kernel": e_got, "torch_f32": e_f32}
        print(f"[gail {label}] net.{k}: kernel {e_got:.3e}  torch f32 {e_f32:.3e}  bound {2.0 * e_f32 + 2e-7:.3e}")
    for k in KEYS:
        assert torch.isfinite(g[k]).all(), (label, k)
        assert out[k]["kernel"] <= 2.0 * out[k]["torch_f32"] + 2e-7, (label, k, out[k])
    return out


FLT_MIN = float(np.finfo(np.float32).tiny)


def check_losses(sums, o64, label):
    """1e-6 relative, each sum.  A row's loss term below f32's smallest normal number (a 30 x network puts -log D of a lone expert
    row at 1e-114) is 0 in ANY f32 evaluation: one FLT_MIN per row is taken off the difference before it is compared."""
    s = sums.cpu().numpy()
    under = len(o64["z"]) * FLT_MIN
    rel = [max(abs(s[i] - o64["loss"][i]) - under, 0.0) / max(abs(o64["loss"][i]), 1e-300) for i in range(2)]
    print(f"[gail {label}] loss sums {s[0]:.9g} {s[1]:.9g} oracle {o64['loss'][0]:.9g} {o64['loss'][1]:.9g} rel {rel[0]:.2e} {rel[1]:.2e}")
    assert rel[0] <= 1e-6 and rel[1] <= 1e-6, (label, rel)
    return rel


def make_rows(ne, npol, od, na, seed):
    rng = np.random.RandomState(seed)
    return (rng.rand(ne, od).astype(np.float32), rng.randint(0, na, ne).astype(np.int32),
            rng.rand(npol, od).astype(np.float32), rng.randint(0, na, npol).astype(np.int32))


def run_grad(ops, flat, rows, na, **kw):
    oe, ae, op_, ap = rows
    return ops.disc_grad(dev(flat), dev(oe), dev(ae), dev(op_), dev(ap), na, **kw)


def saturating_flat(od, na, seed, rows, zmax=200.0):
    """Default-scale first layer; second layer shifted and scaled so that the logits of `rows` span exactly [-zmax, zmax]."""
    flat = default_flat(od, na, seed).double()
    z = oracle(flat, *rows, na)["z"]
    mid = 0.5 * (z.max() + z.min())
    flat[-1] -= mid
    z = z - mid
    flat[-(H + 1):] *= zmax / float(z.abs().max())
    return flat.float()


# ------------------------------------------------------------------------------------------------ 1
def test_oracle_forms_agree_where_nothing_saturates():
    """At nn.Linear's default scale the logit form used as the oracle IS the literal module nn.BCELoss(nn.Sigmoid(...)) in f64:
    loss to 1e-12, gradient to 1e-10 (CPU only; it is here because it pins this file's checker)."""
    od, na = 6, 5
    rows = make_rows(37, 1000, od, na, seed=3)
    flat = default_flat(od, na, seed=4)
    o = oracle(flat, *rows, na)
    assert float(o["z"].abs().max()) < 5.0
    net = checker(flat, od, na, torch.float64)
    de = net(sa_rows(rows[0], rows[1], na, torch.float64))
    dp = net(sa_rows(rows[2], rows[3], na, torch.float64))
    bce = nn.BCELoss()
    le, lp = bce(de, torch.ones_like(de)), bce(dp, torch.zeros_like(dp))
    (le + lp).backward()
    lit = torch.cat([p.grad.reshape(-1) for p in net.parameters()])
    assert abs(float(le.detach()) - o["loss"][0] / 37) <= 1e-12 and abs(float(lp.detach()) - o["loss"][1] / 1000) <= 1e-12
    assert rel_l2(lit, o["grad"]) <= 1e-10


@pytest.mark.parametrize("scale", [1.0, 30.0])
@pytest.mark.parametrize("ne,npol,od", [(1, 3, 6), (37, 1000, 6), (20000, 524288, 6), (37, 1000, 8), (3000, 40001, 8)])
def test_disc_grad_matches_f64(ops, ne, npol, od, scale):
    na = 5
    rows = make_rows(ne, npol, od, na, seed=ne + npol)
    flat = default_flat(od, na, seed=od + int(scale), scale=scale)
    sums, grad = run_grad(ops, flat, rows, na)
    o64, o32 = oracle(flat, *rows, na), oracle(flat, *rows, na, dtype=torch.float32)
    label = f"grad ne={ne} np={npol} od={od} x{scale:g}"
    print(f"[gail {label}] max |z| {float(o64['z'].abs().max()):.1f}")
    rel = check_losses(sums, o64, label)
    errs = check_grad(grad, o64, o32, od, na, label)
    s = sums.cpu().numpy()
    margin = int((o64["z"].abs() < 1e-4 * max(1.0, scale)).sum())          # rows whose f32 logit may fall on the other side of 0
    assert abs(s[2] - o64["correct"]) <= margin and s[3] == 0
    PARITY[label] = {"loss_rel": rel, "grad_rel_l2": errs, "max_abs_logit": float(o64["z"].abs().max())}


# ------------------------------------------------------------------------------------------------ 2
def test_saturated_rows_bad_actions_and_nan_rows(ops):
    od, na, ne, npol = 6, 5, 700, 5000
    rows = list(make_rows(ne, npol, od, na, seed=21))
    flat = saturating_flat(od, na, 22, rows)
    # out-of-range actions: no one-hot column, counted
    rows[1][[3, 77]] = [5, -1]
    rows[3][[0, 4999, 2500]] = [7, -3, 5]
    o64, o32 = oracle(flat, *rows, na), oracle(flat, *rows, na, dtype=torch.float32)
    z = o64["z"]
    assert float(z.max()) > 150 and float(z.min()) < -150
    sums, grad = run_grad(ops, flat, rows, na)
    check_losses(sums, o64, "saturated")
    PARITY["saturated |z| to 200"] = {"grad_rel_l2": check_grad(grad, o64, o32, od, na, "saturated")}
    assert sums[3].item() == 5
    # rows whose own loss term is beyond the clamp: exactly 100 each, nn.BCELoss's clamped value -- and a useful gradient
    t = torch.cat([-z[:ne], z[ne:]])
    far = (t > 102.0).numpy()
    fe, fp = far[:ne], far[ne:]
    assert fe.sum() > 10 and fp.sum() > 10
    sub = (rows[0][fe], rows[1][fe], rows[2][fp], rows[3][fp])
    s_sub, g_sub = run_grad(ops, flat, sub, na)
    assert s_sub[0].item() == 100.0 * fe.sum() and s_sub[1].item() == 100.0 * fp.sum() and s_sub[2].item() == 0
    lit = checker(flat, od, na, torch.float32)                              # the literal f32 module agrees on these rows: 100 each
    bce = nn.BCELoss(reduction="sum")
    with torch.no_grad():
        de, dp = lit(sa_rows(sub[0], sub[1], na, torch.float32)), lit(sa_rows(sub[2], sub[3], na, torch.float32))
        assert float(bce(de, torch.ones_like(de))) == 100.0 * fe.sum() and float(bce(dp, torch.zeros_like(dp))) == 100.0 * fp.sum()
    check_grad(g_sub, oracle(flat, *sub, na), oracle(flat, *sub, na, dtype=torch.float32), od, na, "clamped rows only")
    assert float(g_sub.abs().max()) > 1e-3                                  # torch's BCELoss o Sigmoid backward is 0 here
    # NaN rows (disjoint from the bad actions) are counted too
    rows[0][[10, 11]] = np.nan
    rows[2][[100, 3000, 4000], 2] = np.nan
    s_nan, _ = run_grad(ops, flat, rows, na)
    assert s_nan[3].item() == 5 + 5


# ------------------------------------------------------------------------------------------------ 3
def test_disc_grad_is_deterministic_and_independent_of_the_slab_count(ops):
    from uavppo import _lib
    od, na = 6, 5
    rows = make_rows(3000, 40000, od, na, seed=31)
    flat = default_flat(od, na, seed=32, scale=3.0)
    s1, g1 = run_grad(ops, flat, rows, na)
    s2, g2 = run_grad(ops, flat, rows, na)
    assert torch.equal(g1, g2) and torch.equal(s1, s2)
    o64, o32 = oracle(flat, *rows, na), oracle(flat, *rows, na, dtype=torch.float32)
    h = C.c_void_p()
    _lib.check(_lib.lib().uav_create(C.byref(h), 0, 1 << 20), "uav_create")          # the minimum workspace: fewer slabs
    try:
        s3, g3 = run_grad(ops, flat, rows, na, ctx=h)
        s4, g4 = run_grad(ops, flat, rows, na, ctx=h)
        torch.cuda.synchronize()
    finally:
        _lib.lib().uav_destroy(h)
    assert torch.equal(g3, g4) and torch.equal(s3, s4)
    a = check_grad(g1, o64, o32, od, na, "default workspace")
    b = check_grad(g3, o64, o32, od, na, "minimum workspace")
    check_losses(s3, o64, "minimum workspace")
    assert s1[2].item() == s3[2].item()
    print(f"[gail slabs] bitwise equal across slab counts: {torch.equal(g1, g3)}")
    PARITY["slab count"] = {"default_workspace": a, "minimum_workspace": b}


# ------------------------------------------------------------------------------------------------ 4
@pytest.mark.parametrize("saturate", [False, True])
def test_disc_reward_matches_f64(ops, saturate):
    od, na, n = 6, 5, 100003
    rows = make_rows(1, n, od, na, seed=41)
    flat = saturating_flat(od, na, 42, rows) if saturate else default_flat(od, na, 42)
    obs, act = rows[2], rows[3]
    rew = np.random.RandomState(43).randn(n).astype(np.float32) * 3
    ec, gc = 0.75, 0.3

    def want(dtype, ec, gc):
        with torch.no_grad():
            z = checker(flat, od, na, dtype)[:3](sa_rows(obs, act, na, dtype)).squeeze(1)
            return torch.tensor(ec, dtype=dtype) * torch.as_tensor(rew).to(dtype) + torch.tensor(gc, dtype=dtype) * F.softplus(z), z

    def err(x, ref):
        return float(((x.cpu().double() - ref).abs() / ref.abs().clamp(min=1.0)).max())
    w64, z64 = want(torch.float64, ec, gc)
    w32, _ = want(torch.float32, ec, gc)
    if saturate:
        assert float(z64.max()) > 150 and float(z64.min()) < -150
    got = ops.disc_reward(dev(flat), dev(obs), dev(act), na, gail_coef=gc, env_coef=ec, rew_env=dev(rew))
    e_got, e_f32 = err(got, w64), err(w32, w64)
    print(f"[gail reward saturate={saturate}] kernel {e_got:.3e} torch f32 {e_f32:.3e}")
    assert torch.isfinite(got).all() and e_got <= 2.0 * e_f32 + 2e-7
    PARITY[f"reward saturate={saturate}"] = {"kernel": e_got, "torch_f32": e_f32}
    buf = dev(rew).clone()
    ops.disc_reward(dev(flat), dev(obs), dev(act), na, gail_coef=gc, env_coef=ec, rew_env=buf, out=buf)      # in place
    assert torch.equal(buf, got)
    pure = ops.disc_reward(dev(flat), dev(obs), dev(act), na)                                                  # rew_env NULL: softplus(z)
    p64, p32 = want(torch.float64, 0.0, 1.0)[0], want(torch.float32, 0.0, 1.0)[0]
    print(f"[gail reward saturate={saturate}] softplus alone: kernel {err(pure, p64):.3e} torch f32 {err(p32, p64):.3e}")
    assert err(pure, p64) <= 2.0 * err(p32, p64) + 2e-7


# ------------------------------------------------------------------------------------------------ 5
def _expert(n, seed, od=6):
    rng = np.random.RandomState(seed)
    return rng.rand(n, od).astype(np.float32), rng.randint(0, 5, n).astype(np.int64)


def test_three_discriminator_steps_layered(ops):
    """(a) every step's gradient against the oracle at the trainer's parameters OF THAT STEP; (b) uav_clip_adam(max_norm = 0)
    fed those gradients against torch.optim.Adam fed the same gradients, to one ulp of a parameter.  (No tight comparison of
    free-running trajectories: Adam's first step is lr * sign(g))"""
    from uavppo.gail import GAILTrainer
    lr = 1e-3
    tr = GAILTrainer(64, 32, "lstm", hidden=64, device=DEV, seed=5, use_curriculum=False, expert=_expert(500, 51), disc_steps=3,
                     disc_lr=lr)
    tr.collect()
    tr.record = True
    p0 = tr.disc.flat.clone().cpu()
    tr.update_discriminator()
    assert len(tr.disc_log) == 3 and tr.disc_opt_step == 3
    obs = tr.buf["obs"].reshape(-1, 6).cpu().numpy()
    act = tr.buf["act"].reshape(-1).cpu().numpy()
    rows = (tr.expert_obs.cpu().numpy(), tr.expert_act.cpu().numpy(), obs, act)
    ref = nn.Parameter(p0.clone())
    opt = torch.optim.Adam([ref], lr=lr)
    assert torch.equal(tr.disc_log[0][2].cpu(), p0)
    for i, (sums, grad, params) in enumerate(tr.disc_log):
        o64, o32 = oracle(params.cpu(), *rows, 5), oracle(params.cpu(), *rows, 5, dtype=torch.float32)
        check_losses(sums, o64, f"step {i}")
        PARITY[f"trainer step {i}"] = {"grad_rel_l2": check_grad(grad, o64, o32, 6, 5, f"step {i}")}
        ref.grad = grad.cpu().clone()
        opt.step()
        after = tr.disc_log[i + 1][2].cpu() if i + 1 < 3 else tr.disc.flat.cpu()
        ulp = float(np.spacing(np.float32(ref.detach().abs().max())))
        d = float((after - ref.detach()).abs().max())
        print(f"[gail adam step {i}] max |param diff| {d:.3e}  ulp {ulp:.3e}  moved {float((after - params.cpu()).abs().max()):.3e}")
        assert d <= ulp, (i, d, ulp)
        assert float((after - params.cpu()).abs().max()) > 0.5 * lr          # ... and the step was taken
    el, pl, acc = tr.disc_losses()
    assert np.isfinite([el, pl, acc]).all() and 0.0 <= acc <= 1.0


# ------------------------------------------------------------------------------------------------ 6, 7
@pytest.mark.parametrize("kind,hidden", [("lstm", 64), ("mlp", 128)])
def test_gail_trainer_switched_off_is_the_plain_trainer(kind, hidden):
    from uavppo.gail import GAILTrainer
    from uavppo.trainer import VecPPOTrainer
    a = VecPPOTrainer(64, 32, kind, hidden=hidden, device=DEV, seed=9)
    b = GAILTrainer(64, 32, kind, hidden=hidden, device=DEV, seed=9, expert=_expert(300, 61), env_coef=1.0, gail_coef=0.0)
    d0 = b.disc.flat.clone()
    for _ in range(2):
        a.train_iteration()
        b.train_iteration()
    torch.cuda.synchronize()
    assert torch.equal(a.policy.flat, b.policy.flat) and torch.equal(a.exp_avg, b.exp_avg) and torch.equal(a.exp_avg_sq, b.exp_avg_sq)
    for k in a.buf:
        assert torch.equal(a.buf[k], b.buf[k]), k
    assert a.losses() == b.losses()
    assert not torch.equal(d0, b.disc.flat) and b.disc_opt_step == 2          # the discriminator itself was trained meanwhile


def test_gail_trainer_advantages_are_the_gae_of_the_shaped_reward():
    from uavppo.gail import GAILTrainer
    from uavppo.trainer import VecPPOTrainer
    ec, gc = 0.5, 0.25
    tr = GAILTrainer(64, 32, "lstm", hidden=64, device=DEV, seed=7, use_curriculum=False, expert=_expert(300, 71), env_coef=ec,
                     gail_coef=gc)
    tr.disc.flat.mul_(3.0)                     # logits of a few units, not the +-0.3 of a fresh network
    plain = VecPPOTrainer(64, 32, "lstm", hidden=64, device=DEV, seed=7, use_curriculum=False)
    tr.collect()
    plain.collect()
    tr.compute_advantages()
    b = {k: v.cpu().numpy() for k, v in tr.buf.items()}
    assert np.array_equal(b["rew"], plain.buf["rew"].cpu().numpy())             # buf["rew"] is still the environment's reward
    with torch.no_grad():
        z = checker(tr.disc.flat, 6, 5, torch.float64)[:3](sa_rows(b["obs"].reshape(-1, 6), b["act"].reshape(-1), 5, torch.float64)).squeeze(1)
    assert float(z.abs().max()) > 0.5
    shaped = (ec * torch.as_tensor(b["rew"]).double() + gc * F.softplus(z).reshape(64, 32)).float().numpy()
    assert np.allclose(tr.rew_shaped.cpu().numpy(), shaped, rtol=2e-6, atol=2e-6)       # (the f64 rule itself: test_disc_reward_matches_f64)
    adv = po.gae_reference_exact(shaped, b["val"], b["done"])
    assert np.allclose(tr.adv.cpu().numpy(), adv, rtol=2e-5, atol=2e-5)         # the GAE tolerance of test_gpu_update_kernels.py
    adv_n, ret = po.normalise(adv, b["val"])
    assert np.allclose(tr.adv_n.cpu().numpy().reshape(-1), adv_n.numpy(), atol=2e-5, rtol=1e-4)
    assert not np.allclose(adv, po.gae_reference_exact(b["rew"], b["val"], b["done"]), atol=1e-2)       # the shaping is visible


# ------------------------------------------------------------------------------------------------ 8
def test_discriminator_learns_a_separable_task(ops):
    """Expert action = argmax of a fixed linear map of the state, policy actions uniform; 300 Adam steps at lr 1e-3.  The torch-CPU
    checker alone on this data goes from loss 1.392 / accuracy 0.333 to 0.828 / 0.820 (f64 and f32 alike): room to spare."""
    from model import Discriminator
    g = torch.Generator().manual_seed(0)
    A = torch.randn(6, 5, generator=g)
    se = torch.rand(4096, 6, generator=g)
    ae = ((se - 0.5) @ A).argmax(1)
    sp = torch.rand(8192, 6, generator=g)
    ap = torch.randint(0, 5, (8192,), generator=g)
    disc = Discriminator(6, 5, device=DEV, seed=1)
    m, v = torch.zeros_like(disc.flat), torch.zeros_like(disc.flat)
    rows = [dev(se), dev(ae, torch.int32), dev(sp), dev(ap, torch.int32)]
    hist = []
    for step in range(1, 301):
        sums, _ = ops.disc_grad(disc.flat, *rows, 5, grad=disc.grad)
        if step in (1, 300):
            s = sums.cpu().numpy()
            hist.append((s[0] / 4096 + s[1] / 8192, s[2] / (4096 + 8192)))
            assert s[3] == 0
        ops.clip_adam(disc.flat, disc.grad, m, v, step, 1e-3, max_norm=0.0)
    print(f"[gail learn] loss {hist[0][0]:.4f} -> {hist[1][0]:.4f}, accuracy {hist[0][1]:.3f} -> {hist[1][1]:.3f}")
    assert hist[1][0] < hist[0][0] and hist[1][1] > 0.5
    # the reference's call surface on the trained network: D [n, 1] from one-hot actions, higher on expert pairs
    de = disc(se[:512], F.one_hot(ae[:512], 5).float())
    dp = disc(sp[:512], ap[:512])
    assert tuple(de.shape) == (512, 1) and de.device.type == "cpu" and float(de.mean()) > float(dp.mean())
    ref = checker(disc.flat, 6, 5, torch.float64)
    ref.load_state_dict({f"{k[4:]}": t.double().cpu() for k, t in disc.state_dict().items()})          # keys net.0.weight ... load into the module
    with torch.no_grad():
        assert torch.allclose(de.double(), ref(sa_rows(se[:512], ae[:512], 5, torch.float64)), atol=1e-6, rtol=1e-5)


def test_compute_discriminator_loss_and_state_dict_round_trip(ops):
    import model
    tm = nn.Module()
    tm.net = nn.Sequential(nn.Linear(11, H), nn.ReLU(), nn.Linear(H, 1), nn.Sigmoid())
    disc = model.Discriminator(state_dim=6, action_dim=5)
    assert sorted(disc.state_dict()) == sorted(tm.state_dict())
    torch.manual_seed(5)
    tm2 = nn.Sequential(nn.Linear(11, H), nn.ReLU(), nn.Linear(H, 1), nn.Sigmoid())
    disc.load_state_dict({"net." + k: v for k, v in tm2.state_dict().items()})          # from the torch module ...
    tm.load_state_dict(disc.state_dict())                                                  # ... and into it
    for k, v in tm2.state_dict().items():
        assert torch.equal(tm.state_dict()["net." + k], v)
    oe, ae, op_, ap = make_rows(100, 400, 6, 5, seed=81)
    ap[:] = np.minimum(ap, 3)                   # the largest action is absent from the policy batch: the reference's one-hot width breaks here
    loss = model.compute_discriminator_loss(disc, torch.as_tensor(oe), torch.as_tensor(ae).long(), torch.as_tensor(op_), torch.as_tensor(ap).long())
    o64 = oracle(disc.flat, oe, ae, op_, ap, 5)
    assert loss.dim() == 0 and abs(float(loss) - (o64["loss"][0] / 100 + o64["loss"][1] / 400)) <= 1e-6
    check_grad(disc.grad, o64, oracle(disc.flat, oe, ae, op_, ap, 5, dtype=torch.float32), 6, 5, "compute_discriminator_loss")


# ------------------------------------------------------------------------------------------------ 9
def _direct_pairs(ops, core, hidden, N, seed, steps):
    """Pairs cut by a plain per-env loop from ONE direct uav_greedy_episodes launch."""
    from uavppo.vec_env import VecMethaneEnv
    env = VecMethaneEnv(N, "v2.0", DEV, seed=seed)
    env.reset()
    cur0 = env.obs.cpu().numpy().copy()
    h = torch.zeros(N, hidden, device=DEV) if hidden else None
    c = torch.zeros(N, hidden, device=DEV) if hidden else None
    active = torch.ones(N, dtype=torch.uint8, device=DEV)
    recs = {"act": torch.empty(N, steps, dtype=torch.int32, device=DEV), "obs": torch.empty(N, steps, 6, device=DEV),
            "pos": torch.empty(N, steps, 2, device=DEV), "flags": torch.empty(N, steps, dtype=torch.uint8, device=DEV)}
    ops.greedy_episodes(env.state, N, env.cfg(), core.flat, hidden, steps, env.obs, h, c, active, recs)
    obs, act, flags = recs["obs"].cpu().numpy(), recs["act"].cpu().numpy(), recs["flags"].cpu().numpy()
    S, A, lengths = [], [], []
    for n in range(N):
        state, L = cur0[n], 0
        for t in range(steps):
            if flags[n, t] & 4:
                break
            S.append(state)
            A.append(act[n, t])
            state, L = obs[n, t], L + 1
        lengths.append(L)
    return np.array(S, dtype=np.float32), np.array(A, dtype=np.int64), lengths


@pytest.mark.parametrize("kind", ["mlp", "lstm"])
def test_generate_expert_data_equals_a_direct_greedy_run(ops, kind, tmp_path):
    import generate_expert_data as ged
    import model
    from uavppo.policy import LSTMActorCritic
    N, steps, seed = 24, 300, 77
    if kind == "mlp":
        pol = model.PPOActorCritic(6, 5, device=DEV)
        core, hidden = pol.core, 0
        core.views["head.weight"][:5].mul_(100.0)
    else:
        pol = core = LSTMActorCritic(6, 128, 1, device=DEV, seed=3)
        hidden = 128
        core.views["head.weight"][:5].mul_(400.0)            # a decisive greedy policy
    out = str(tmp_path / "expert_data.npz")
    states, actions = ged.generate_expert_data(pol, num_episodes=N, variant="v2.0", seed=seed, max_steps=steps, out=out)      # chunks of 250 + 50
    S, A, lengths = _direct_pairs(ops, core, hidden, N, seed, steps)
    print(f"[gail expert {kind}] episode lengths {lengths}")
    assert len(actions) == sum(lengths) > 0
    assert np.array_equal(states, S) and np.array_equal(actions, A)
    assert states.dtype == np.float32 and actions.dtype == np.int64 and actions.min() >= 0 and actions.max() < 5
    s, a = model.get_expert_data(out)
    assert np.array_equal(s.numpy(), S) and np.array_equal(a.numpy(), A)
    # a checkpoint as train_ppo2.0.py writes it loads into the same policy
    ck = str(tmp_path / "policy.pth")
    torch.save({k: v.cpu() for k, v in pol.state_dict().items()}, ck)
    s2, a2 = ged.generate_expert_data(ck, num_episodes=N, variant="v2.0", seed=seed, max_steps=steps, out=None, device=DEV)
    assert np.array_equal(s2, S) and np.array_equal(a2, A)


def test_generate_expert_data_stepwise_path_cuts_the_same_records(ops):
    """Where the fused kernel refuses the policy (here: two layers) the step-wise loop leaves records of the same format: the pairs
    replay against a direct step-by-step run of the same policy and environment."""
    import generate_expert_data as ged
    from evaluate_with_lstm import fused_refusal
    from uavppo.policy import LSTMActorCritic
    from uavppo.vec_env import VecMethaneEnv
    N, steps, seed = 12, 120, 5
    pol = LSTMActorCritic(6, 64, 2, device=DEV, seed=2)
    pol.views["head.weight"][:5].mul_(400.0)
    assert fused_refusal(pol, VecMethaneEnv(N, "v2.0", DEV, seed=seed)) is not None
    states, actions = ged.generate_expert_data(pol, num_episodes=N, seed=seed, max_steps=steps, out=None)
    env = VecMethaneEnv(N, "v2.0", DEV, seed=seed)
    obs = env.reset()
    h, c = pol.zero_state(N)
    live = np.ones(N, bool)
    per_env = [([], []) for _ in range(N)]
    work = {}
    for _ in range(steps):
        act = pol.step(obs, h, c, work=work)[:, :5].argmax(1).to(torch.int32)
        o_np, a_np = obs.cpu().numpy().copy(), act.cpu().numpy()
        obs, _, done, _ = env.step(act)
        for n in np.nonzero(live)[0]:
            per_env[n][0].append(o_np[n])
            per_env[n][1].append(a_np[n])
        live &= ~(done.cpu().numpy() > 0.5)
    S = np.array([s for e in per_env for s in e[0]], dtype=np.float32)
    A = np.array([a for e in per_env for a in e[1]], dtype=np.int64)
    assert np.array_equal(states, S) and np.array_equal(actions, A)


# ------------------------------------------------------------------------------------------------ 10
def test_train_ppo_gail_script_smoke(tmp_path):
    es, ea = _expert(400, 91)
    np.savez(str(tmp_path / "expert_data.npz"), states=es, actions=ea)
    env = dict(os.environ)
    cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.join(PKG, "train_ppo_gail.py"), "--episodes", "1000000",
           "--max-iterations", "3", "--num-envs", "64", "--horizon", "32", "--policy", "lstm", "--hidden", "64"]
    r = subprocess.run(cmd, cwd=str(tmp_path), env=env, capture_output=True, text=True)          # a fresh child process under its own limit
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0
    assert "Episode 0 | Mean Reward:" in r.stdout and "Success Rate:" in r.stdout
    line = [ln for ln in r.stdout.splitlines() if "D expert" in ln][0].split()
    vals = [float(line[line.index(k) + 1]) for k in ("expert", "policy", "accuracy")]
    assert np.isfinite(vals).all() and 0.0 <= vals[2] <= 1.0
    pol = torch.load(str(tmp_path / "ppo_gail_model.pth"), map_location="cpu")
    dsc = torch.load(str(tmp_path / "discriminator.pth"), map_location="cpu")
    assert any(k.startswith("lstm.") for k in pol) and sorted(dsc) == ["net.0.bias", "net.0.weight", "net.2.bias", "net.2.weight"]
    assert tuple(dsc["net.0.weight"].shape) == (128, 11) and all(torch.isfinite(v).all() for v in dsc.values())
