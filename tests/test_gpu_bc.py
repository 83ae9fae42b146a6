"""Behaviour cloning on the GPU: uav_bc_loss and uav_mlp_bc_grad against the f64 oracle of tests/test_bc_host.py (bc_oracle on
top of oracle.ppo_oracle's forward passes and torch-CPU autograd), the rows form against the contiguous form, the LSTM route,
BCTrainer end to end, the refusals and the hand-over to the scripts that load a checkpoint.  -m gpu.

Shapes: n = 1, a partial 32-sample tile (7), two tiles with a partial one (33), several workgroups (100), workgroups that loop
over two tiles (8300 > 256 CUs x 32); 257 = one 256-thread block + 1 and 5000 = 20 blocks for the element-wise kernel; ragged
episodes of odd lengths.  Tolerances are those of the tests each case restates (test_gpu_trend_mlp.py, test_gpu_inline_update.py,
test_gpu_trainer.py), quoted where they are used."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from oracle import ppo_oracle as po
from test_bc_host import bc_oracle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "uav-wrf-les-ppo-lstm_amd")
TOWARDS = [0.0, 2.0, -5.0, 2.0, -5.0]       # head bias of the hand-made teacher: walks +x / +y (tests/test_gpu_greedy_eval.py's recipe)
GAP = 1e-4                                  # logits closer than this may order differently in f32 and f64
LR = 3e-5                                   # the step size of the update tests whose parameter bound (atol 3e-6) is used here


def d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def p64(pol):
    return {k: v.detach().cpu().double() for k, v in pol.named_views().items()}


def named_from_flat(pol, flat):
    """{reference key: tensor} views of a flat vector in the layout of pol.flat (what pol.named_grads() is for pol.grad)."""
    out, o = {}, 0
    for name, shape in pol.layout:
        n = int(np.prod(shape))
        out[name] = flat[o:o + n].view(shape)
        o += n
    return pol._named(out)


def towards_mlp(seed, k=0, scale=400.0):
    """A decisive hand-made MLP (the "towards the source" construction of tests/test_gpu_trend_mlp.py::_trend_mlp, rebuilt):
    actor rows of gain 0.01 scaled up, a head bias that walks +x / +y."""
    from uavppo.policy import MLPActorCritic
    pol = MLPActorCritic(6 + k, 5, device=DEV, seed=seed)
    pol.views["head.weight"][:5].mul_(scale)
    pol.views["head.bias"][:5].copy_(torch.tensor(TOWARDS))
    if k:
        pol.views["feature.0.weight"][:, 6:].mul_(20.0)
    return pol


def busy_mlp(D, seed):
    """test_fused_trend_mlp_gradient_matches_oracle_and_layered_path's preparation: non-trivial LayerNorm parameters and biases,
    head weights x 20."""
    from uavppo.policy import MLPActorCritic
    pol = MLPActorCritic(D, 5, device=DEV, seed=seed)
    with torch.no_grad():
        g = torch.Generator().manual_seed(1)
        for key in ("feature.0.bias", "feature.1.bias", "feature.3.bias", "feature.4.bias", "head.bias"):
            pol.views[key].copy_(torch.randn(pol.views[key].shape, generator=g) * 0.2)
        for key in ("feature.1.weight", "feature.4.weight"):
            pol.views[key].copy_(1 + 0.3 * torch.randn(pol.views[key].shape, generator=g))
        pol.views["head.weight"].mul_(20.0)
    return pol


def mlp_oracle_grad(params64, obs, act, vt, vcoef, beta):
    """f64 autograd of the cloning loss through the MLP: ({key: gradient}, sums)."""
    leaf = {k: v.clone().requires_grad_(True) for k, v in params64.items()}
    _, value, logits = po.mlp_forward(leaf, torch.from_numpy(np.asarray(obs, np.float64)))
    total, sums = bc_oracle(logits, value[:, 0], torch.from_numpy(np.asarray(act)),
                            None if vt is None else torch.from_numpy(np.asarray(vt, np.float64)), vcoef, beta)
    total.backward()
    return {k: (leaf[k].grad if leaf[k].grad is not None else torch.zeros_like(leaf[k])) for k in leaf}, [float(s.detach()) for s in sums]


# ---------------------------------------------------------------------------------------------- 1. uav_bc_loss
def _loss_case(n, seed):
    rng = np.random.RandomState(seed)
    heads = rng.randn(n, 6).astype(np.float32)
    heads[:, :5] *= rng.uniform(0.5, 12.0, (n, 1)).astype(np.float32)          # some rows nearly one-hot
    act = rng.randint(0, 5, n).astype(np.int32)
    act[2::3] = -1                                                              # a third of the rows masked
    if n >= 7:
        act[1] = 5                                                              # out of range on the other side: masked too
        heads[3, :5] = [30.0, 0.0, 0.0, 0.0, 0.0]                               # q[a] = e^-30 < eps: the clamp binds
        act[3] = 4
        heads[4, :5] = [0.0, 25.0, 0.0, 0.0, 0.0]                               # q[a] > 1 - eps: binds from above
        act[4] = 1
    vt = rng.randn(n).astype(np.float32)
    return heads, act, vt


@pytest.mark.parametrize("with_vt,beta,vcoef", [(False, 0.0, 0.0), (True, 0.01, 0.5), (False, 0.01, 0.5), (True, 0.0, 0.5)])
@pytest.mark.parametrize("n", [1, 7, 257, 5000])
def test_bc_loss_matches_f64_oracle(n, with_vt, beta, vcoef):
    from uavppo import ops
    heads, act, vt = _loss_case(n, n)
    if not with_vt:
        vt = None
    valid = (act >= 0) & (act < 5)
    cnt = int(valid.sum())
    inv_n = 1.0 / cnt
    h64 = torch.from_numpy(heads.astype(np.float64)).requires_grad_(True)
    total, sums = bc_oracle(h64[:, :5], h64[:, 5], torch.from_numpy(act), None if vt is None else torch.from_numpy(vt.astype(np.float64)),
                            vcoef, beta)
    total.backward()
    want = h64.grad.numpy()
    out = []
    for _ in range(2):
        s = torch.full((6,), -1.0, dtype=torch.float64, device=DEV)
        dh = torch.full((n, 6), float("nan"), device=DEV)
        db = torch.full((6,), float("nan"), device=DEV)
        ops.bc_loss_heads(d(heads), d(act), None if vt is None else d(vt), inv_n, vcoef, beta, s, dh, db)
        out.append((s.cpu().numpy(), dh.cpu().numpy(), db.cpu().numpy()))
    (s, dh, db), (s2, dh2, db2) = out
    assert np.array_equal(s, s2) and np.array_equal(dh, dh2) and np.array_equal(db, db2)         # a fixed reduction order
    print("sums", s, [float(x) for x in sums])
    assert np.allclose(s[:3] / cnt, [float(sums[0]) / cnt, float(sums[1]) / cnt, float(sums[2]) / cnt], rtol=2e-5, atol=1e-6)
    assert s[3] == 0 and s[4] == float(sums[3]) and s[5] == cnt
    assert (dh[~valid] == 0).all()
    # test_gpu_inline_update.py's bound for the loss sums, per column of dheads
    err = np.abs(dh - want)
    tol = 1e-6 * np.abs(want).max(0, keepdims=True) + 2e-5 * np.abs(want)
    print("dheads max err / tol", (err / (tol + 1e-300)).max())
    assert (err <= tol).all(), (err - tol).max()
    if vt is None or vcoef == 0:
        assert (dh[:, 5] == 0).all()
    if n >= 7 and beta == 0:
        assert (dh[3, :5] == 0).all() and (dh[4, :5] == 0).all()                              # the clamp binds: no policy gradient
    col = dh.astype(np.float64).sum(0)
    assert (np.abs(db - col) <= 2.0 ** -23 * np.abs(dh.astype(np.float64)).sum(0) + 1e-30).all(), (db, col)


def test_bc_entries_leave_an_attached_diagnostics_buffer_alone():
    from uavppo import ops
    heads, act, vt = _loss_case(257, 3)
    diag = torch.full((ops.PPO_DIAG_N,), 7.0, dtype=torch.float64, device=DEV)
    s = torch.zeros(6, dtype=torch.float64, device=DEV)
    pol = busy_mlp(6, 2)
    rng = np.random.RandomState(0)
    obs, a = d(rng.rand(100, 6).astype(np.float32)), d(rng.randint(0, 5, 100).astype(np.int32))
    g0 = torch.empty_like(pol.flat)
    ops.mlp_bc_grad(pol.flat, obs, a, None, 0.01, 0.0, 0.0, s, g0)
    s0 = s.clone()
    ops.set_ppo_diag(diag)
    try:
        ops.bc_loss_heads(d(heads), d(act), d(vt), 1.0 / 257, 0.5, 0.01, s, torch.empty(257, 6, device=DEV))
        g1 = torch.empty_like(pol.flat)
        ops.mlp_bc_grad(pol.flat, obs, a, None, 0.01, 0.0, 0.0, s, g1)
        torch.cuda.synchronize()
    finally:
        ops.set_ppo_diag(None, DEV)
    assert (diag == 7.0).all() and torch.equal(g0, g1) and torch.equal(s0, s)


# ---------------------------------------------------------------------------------------------- 2. uav_mlp_bc_grad
@pytest.mark.parametrize("mode", ["fp16x3", "f32_mfma"])
@pytest.mark.parametrize("k", [0, 1, 2])
@pytest.mark.parametrize("n", [1, 7, 33, 100, 8300])
def test_fused_mlp_bc_gradient_matches_oracle_and_layered_path(n, k, mode):
    """test_fused_trend_mlp_gradient_matches_oracle_and_layered_path with the cloning loss (no kink redraw: the loss has no kink
    away from the clamp), with masked samples, without and with value targets."""
    from uavppo import ops
    D = 6 + k
    pol = busy_mlp(D, n)
    rng = np.random.RandomState(n + k)
    obs = rng.rand(n, D).astype(np.float32)
    obs[:, 6:] = (0.05 * rng.randn(n, k)).astype(np.float32)
    act = rng.randint(0, 5, n).astype(np.int32)
    if n > 1:
        act[1::4] = -1
    vt_all = rng.randn(n).astype(np.float32)
    cnt = int(((act >= 0) & (act < 5)).sum())
    params = p64(pol)
    bound = lambda scale: (2e-5 + 2e-7 * np.sqrt(n)) * scale + 1e-9             # that test's bound: f32 sums over n samples in another order
    for vt, vcoef, beta in ((None, 0.0, 0.0), (vt_all, 0.5, 0.01)):
        sums = torch.zeros(6, dtype=torch.float64, device=DEV)
        pol.grad.fill_(float("nan"))
        with ops.lstm_arith(mode):
            ops.mlp_bc_grad(pol.flat, d(obs), d(act), None if vt is None else d(vt), 1.0 / cnt, vcoef, beta, sums, pol.grad, trend_k=k)
            got = {key: v.detach().cpu().double() for key, v in pol.named_grads().items()}
            got_flat = pol.grad.clone()
        s = sums.cpu().numpy()
        want, wsums = mlp_oracle_grad(params, obs, act, vt, vcoef, beta)
        print("sums", s, wsums)
        assert np.allclose(s[:3] / cnt, np.array(wsums[:3]) / cnt, rtol=2e-5, atol=1e-6) and s[3] == 0 and s[5] == cnt
        assert abs(s[4] - wsums[3]) <= _near_ties(params, obs, act)
        for key in want:
            scale = want[key].abs().max().item() + 1e-12
            err = (got[key] - want[key]).abs().max().item()
            print(key, "err", err, "bound", bound(scale))
            assert err <= bound(scale), (key, err, scale)
        if vt is None:
            assert (got["critic.weight"] == 0).all() and (got["critic.bias"] == 0).all()
        # layer-by-layer HIP path
        heads = pol.heads(d(obs))
        dheads = torch.empty(n, 6, device=DEV)
        s2 = torch.zeros(6, dtype=torch.float64, device=DEV)
        ops.bc_loss_heads(heads, d(act), None if vt is None else d(vt), 1.0 / cnt, vcoef, beta, s2, dheads)
        g2 = pol.backward(dheads).clone()
        print("layered max diff", (got_flat - g2).abs().max().item(), "max|g|", g2.abs().max().item())
        assert torch.allclose(got_flat, g2, rtol=2e-4, atol=2e-6 * g2.abs().max().item())
        s2 = s2.cpu().numpy()
        assert np.allclose(s[:3], s2[:3], rtol=2e-5) and s[3] == s2[3] and s[5] == s2[5] and abs(s[4] - s2[4]) <= _near_ties(params, obs, act)


def _near_ties(params, obs, act):
    """Samples whose two largest f64 logits are closer than GAP: their argmax may differ between f32 paths."""
    with torch.no_grad():
        lg = po.mlp_forward(params, torch.from_numpy(np.asarray(obs, np.float64)))[2]
    top = lg.topk(2, -1)[0]
    return int(((top[:, 0] - top[:, 1]) < GAP).sum())


# ---------------------------------------------------------------------------------------------- 3. rows form
@pytest.mark.parametrize("mode", ["fp16x3", "f32_mfma"])
@pytest.mark.parametrize("k", [0, 2])
def test_bc_rows_form_is_the_contiguous_form_on_gathered_rows(k, mode):
    """As uav_mlp_ppo_grad_rows promises: bit-identical gradient and sums.  An index outside [0, n_total) is clamped by the
    kernel's row_of before any address is formed, so the bad-index case reads inside the buffers by construction."""
    from uavppo import ops
    n_total, D = 1000, 6 + k
    pol = busy_mlp(D, 4)
    rng = np.random.RandomState(k)
    obs = rng.rand(n_total, D).astype(np.float32)
    act = rng.randint(0, 5, n_total).astype(np.int32)
    act[5::7] = -1
    vt = rng.randn(n_total).astype(np.float32)
    perm = rng.permutation(n_total).astype(np.int32)
    repeated = perm[:333].copy()
    repeated[10] = repeated[11] = repeated[200]
    outside = perm[333:666].copy()
    outside[0], outside[1], outside[40] = -3, n_total, n_total + 12345
    for rows in (perm[:333], repeated, outside, perm[666:]):
        src = np.clip(rows, 0, n_total - 1)
        res = []
        for form in ("rows", "contiguous"):
            sums = torch.zeros(6, dtype=torch.float64, device=DEV)
            grad = torch.full_like(pol.flat, float("nan"))
            with ops.lstm_arith(mode):
                if form == "rows":
                    ops.mlp_bc_grad(pol.flat, d(obs), d(act), d(vt), 1.0 / len(rows), 0.5, 0.01, sums, grad, trend_k=k, rows=d(rows))
                else:
                    ops.mlp_bc_grad(pol.flat, d(obs[src]), d(act[src]), d(vt[src]), 1.0 / len(rows), 0.5, 0.01, sums, grad, trend_k=k)
            res.append((grad.cpu(), sums.cpu()))
        assert torch.isfinite(res[0][0]).all() and (res[0][0] != 0).any()
        assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
        assert res[0][1][5] == ((act[src] >= 0) & (act[src] < 5)).sum()


# ---------------------------------------------------------------------------------------------- 4. LSTM route
LENGTHS = [1, 3, 11, 11, 5, 8, 2]


def _episodes(seed, D=6):
    rng = np.random.RandomState(seed)
    M = sum(LENGTHS)
    states = rng.rand(M, D).astype(np.float32)
    actions = rng.randint(0, 5, M).astype(np.int64)
    vt = rng.randn(M).astype(np.float32)
    return states, actions, np.array(LENGTHS, np.int64), vt


def lstm_oracle_grad(params64, states, actions, lengths, vt, vcoef, beta):
    """f64 autograd of the cloning loss over UNPADDED episodes: each one its own forward pass of its own length from a zero state."""
    leaf = {k: v.clone().requires_grad_(True) for k, v in params64.items()}
    L, H = sum(1 for k in leaf if k.startswith("lstm.weight_ih_l")), leaf["lstm.weight_hh_l0"].shape[1]
    lg, val, o = [], [], 0
    for n in lengths:
        x = torch.from_numpy(states[o:o + n].astype(np.float64))[:, None, :]
        z = torch.zeros(L, 1, H, dtype=torch.float64)
        _, value, logits, _ = po.lstm_policy_forward(leaf, x, z, z.clone())
        lg.append(logits[:, 0])
        val.append(value[:, 0])
        o += n
    total, sums = bc_oracle(torch.cat(lg), torch.cat(val), torch.from_numpy(actions), None if vt is None else torch.from_numpy(vt.astype(np.float64)),
                            vcoef, beta)
    total.backward()
    return {k: (leaf[k].grad if leaf[k].grad is not None else torch.zeros_like(leaf[k])) for k in leaf}, [float(s.detach()) for s in sums]


@pytest.mark.parametrize("H,L", [(64, 1), (128, 2), (256, 2)])
def test_lstm_bc_steps_match_f64_oracle(H, L):
    """Three optimiser steps of BCTrainer on 7 ragged episodes padded to 11 against f64 autograd through lstm_policy_forward and
    an f64 Adam, at test_lstm_ppo_update_matches_oracle's per-step bounds: sums rtol 2e-4 / atol 2e-6, gradient norm rtol 2e-3,
    parameters atol 3e-6 after the steps.  The first step's gradient is also compared tensor by tensor at the norm's bound,
    2e-3 of the tensor's largest element: the same relative bound, applied where a tensor's own rounding shows."""
    from uavppo.bc import BCTrainer
    from uavppo.policy import LSTMActorCritic
    states, actions, lengths, vt = _episodes(H + L)
    pol = LSTMActorCritic(6, H, L, 5, DEV, seed=3)
    pol.views["head.weight"][:5].mul_(30.0)
    tr = BCTrainer(pol, (states, actions, lengths), batch=7, lr=LR, value_coef=0.5, ent_beta=0.01, value_targets=vt)
    assert tr.obs.shape == (7, 11, 6) and tr.act.shape == (7, 11)
    tr.record = True
    tr.forced_perms = [torch.arange(7) for _ in range(3)]
    p = p64(pol)
    adam = po.AdamState(p, lr=LR)
    n = sum(LENGTHS)
    for step in range(3):
        tr.epoch()
        want, wsums = lstm_oracle_grad(p, states, actions, lengths, vt, 0.5, 0.01)
        s, gn, grad, _ = tr.log[step]
        s = s.cpu().numpy()
        print("step", step, "sums", s, wsums)
        assert np.allclose(s[:3] / n, np.array(wsums[:3]) / n, rtol=2e-4, atol=2e-6) and s[3] == 0 and s[5] == n
        if step == 0:
            got = named_from_flat(pol, grad.cpu().double())
            for key in want:
                scale = want[key].abs().max().item()
                err = (got[key] - want[key]).abs().max().item()
                print(key, "err", err, "bound", 2e-3 * scale)
                assert err <= 2e-3 * scale + 1e-12, (key, err, scale)
        grads = {k: v.clone() for k, v in want.items()}
        gnorm = po.clip_grads(grads)
        assert np.isclose(gn.item(), gnorm, rtol=2e-3), (step, gn.item(), gnorm)
        adam.step(p, grads)
    got = p64(pol)
    for k in p:
        assert torch.allclose(got[k], p[k], atol=3e-6, rtol=0), (k, (got[k] - p[k]).abs().max().item())
    m = tr.metrics()
    assert m["samples"] == n and np.isclose(m["nll"], wsums[0] / n, rtol=2e-4)


def test_lstm_bc_gradient_ignores_what_padded_steps_hold():
    """NaN observations in the padded steps of the resident set: the gradient is the one without them, bit for bit, and so
    the unpadded oracle's.  This holds only because padding comes AFTER an episode's last real step -- a padded step feeds no
    real one through the recurrence, the loss masks its heads, and the LSTM route zeroes its input before the forward pass
    (0 x NaN would otherwise reach the weight gradients through the gate derivatives)."""
    from uavppo.bc import BCTrainer
    from uavppo.policy import LSTMActorCritic
    states, actions, lengths, vt = _episodes(9)
    grads = []
    for poison in (False, True):
        pol = LSTMActorCritic(6, 64, 1, 5, DEV, seed=3)
        tr = BCTrainer(pol, (states, actions, lengths), batch=7, lr=LR)
        if poison:
            for e, n in enumerate(LENGTHS):
                tr.obs[e, n:] = float("nan")
        chunk = torch.arange(7, device=DEV)
        grads.append(tr.grad_of(chunk, sum(LENGTHS)).clone())
        s = tr.bc_sums.cpu().numpy()
        assert s[3] == 0 and s[5] == sum(LENGTHS)
    assert torch.isfinite(grads[1]).all() and torch.equal(grads[0], grads[1])
    want, _ = lstm_oracle_grad(p64(pol), states, actions, lengths, None, 0.0, 0.0)
    got = named_from_flat(pol, grads[1].cpu().double())
    for key in want:
        scale = want[key].abs().max().item()
        assert (got[key] - want[key]).abs().max().item() <= 2e-3 * scale + 1e-12, key


# ---------------------------------------------------------------------------------------------- 5. BCTrainer, MLP
def _teacher_set(n=2048, seed=11):
    """n random observations labelled by the greedy action of the hand-made teacher, from its f64 logits."""
    rng = np.random.RandomState(seed)
    obs = rng.rand(n, 6).astype(np.float32)
    teacher = towards_mlp(7)
    with torch.no_grad():
        lg = po.mlp_forward(p64(teacher), torch.from_numpy(obs.astype(np.float64)))[2]
    return obs, lg.argmax(-1).numpy().astype(np.int64)


def cpu_bc_loop(params64, obs, act, perms, batch, lr=LR, vcoef=0.0, beta=0.0):
    """BCTrainer's MLP loop in torch-CPU f64: per step (sums, gradient norm); params64 updated in place."""
    adam = po.AdamState(params64, lr=lr)
    log = []
    for perm in perms:
        for rows in torch.as_tensor(perm).split(batch):
            r = rows.numpy()
            grads, sums = mlp_oracle_grad(params64, obs[r], act[r], None, vcoef, beta)
            gn = po.clip_grads(grads)
            adam.step(params64, grads)
            log.append(sums + [gn])
    return np.array(log)


@pytest.mark.parametrize("batch,epochs", [(512, 3), (500, 1)])
def test_bc_trainer_mlp_matches_cpu_loop_and_learns(batch, epochs):
    """2048 pairs labelled by a fixed teacher; every step's sums and gradient norm and the final parameters against the same
    loop in f64 (bounds of the gradient test: sums rtol 2e-5 / atol 1e-6; norm rtol 2e-3 and parameters atol 3e-6 as
    test_gpu_trainer.py's update tests).  batch = 500 leaves a last chunk of 48 rows: a wrong inv_n there scales its gradient
    norm by 500 / 48.  The CPU loop alone, with these seeds, gives nll 1.610659, 1.603425, 1.596307 and accuracy 0.0981, 0.2344,
    0.7095 over the three epochs at batch 512 (checked before relying on the two learning conditions)."""
    from uavppo.bc import BCTrainer
    from uavppo.policy import MLPActorCritic
    obs, act = _teacher_set()
    pol = MLPActorCritic(6, 5, device=DEV, seed=5)
    g = torch.Generator().manual_seed(3)
    perms = [torch.randperm(2048, generator=g) for _ in range(epochs)]
    p = p64(pol)
    tr = BCTrainer(pol, (obs, act), batch=batch, lr=LR)
    assert tr.fused_mlp
    tr.record = True
    tr.forced_perms = [x.clone() for x in perms]
    ms = []
    for _ in range(epochs):
        tr.epoch()
        ms.append(tr.metrics())
    log = cpu_bc_loop(p, obs, act, perms, batch)
    steps = -(-2048 // batch) * epochs
    assert len(tr.log) == steps == len(log)
    sizes = [len(c) for _ in range(epochs) for c in torch.arange(2048).split(batch)]
    for i, (s, gn, _, _) in enumerate(tr.log):
        s = s.cpu().numpy()
        assert s[5] == sizes[i] and s[3] == 0
        assert np.allclose(s[:3] / sizes[i], log[i, :3] / sizes[i], rtol=2e-5, atol=1e-6), (i, s, log[i])
        assert abs(s[4] - log[i, 3]) <= 2, (i, s[4], log[i, 3])                 # a near-tie of two logits may flip an argmax
        assert np.isclose(gn.item(), log[i, 5], rtol=2e-3), (i, gn.item(), log[i, 5])
    got = p64(pol)
    for k in p:
        assert torch.allclose(got[k], p[k], atol=3e-6, rtol=0), (k, (got[k] - p[k]).abs().max().item())
    per = len(log) // epochs
    for e, m in enumerate(ms):
        blk = log[e * per:(e + 1) * per]
        assert m["samples"] == 2048 and np.isclose(m["nll"], blk[:, 0].sum() / 2048, rtol=2e-5)
    print("metrics", ms)
    if epochs > 1:
        assert ms[-1]["nll"] < ms[0]["nll"] and ms[-1]["accuracy"] >= ms[0]["accuracy"]


def test_bc_trainer_layered_route_agrees_with_the_fused_one():
    """fused_mlp = False sends the same policy down heads() + uav_bc_loss + backward(): one epoch, same permutation, the two
    routes' parameters within the update tests' atol 3e-6."""
    from uavppo.bc import BCTrainer
    from uavppo.policy import MLPActorCritic
    obs, act = _teacher_set(600, 2)
    out = []
    for fused in (True, False):
        pol = MLPActorCritic(6, 5, device=DEV, seed=5)
        tr = BCTrainer(pol, (obs, act), batch=256, lr=LR, ent_beta=0.01)
        tr.fused_mlp = fused
        tr.guard.enabled = fused
        tr.forced_perms = [torch.arange(600).flip(0)]
        tr.epoch()
        out.append((pol.flat.clone(), tr.metrics()))
    assert torch.allclose(out[0][0], out[1][0], atol=3e-6, rtol=0)
    assert np.isclose(out[0][1]["nll"], out[1][1]["nll"], rtol=2e-5) and out[0][1]["samples"] == out[1][1]["samples"] == 600


# ---------------------------------------------------------------------------------------------- 6. refusals
def test_refusals_run_nothing():
    from uavppo import _lib, ops
    lib = _lib.lib()
    h = ops.Context.get(DEV).handle
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    n = 64
    heads, act = torch.randn(n, 6, device=DEV), torch.zeros(n, dtype=torch.int32, device=DEV)
    sums = torch.full((6,), -1.0, dtype=torch.float64, device=DEV)
    dheads = torch.full((n, 6), 5.0, device=DEV)
    pol = busy_mlp(6, 1)
    obs = torch.rand(n, 6, device=DEV)
    grad = torch.full_like(pol.flat, 5.0)

    def refused(rc):
        assert rc != 0 and len(lib.uav_last_error()) > 0
        torch.cuda.synchronize()
        assert (dheads == 5.0).all() and (grad == 5.0).all() and (sums == -1.0).all()

    refused(lib.uav_bc_loss(h, ptr(heads), ptr(act), None, n, 4, 1.0 / n, 0.0, 0.0, ptr(sums), ptr(dheads), None, st))
    refused(lib.uav_bc_loss(h, ptr(heads), ptr(act), None, 0, 5, 1.0, 0.0, 0.0, ptr(sums), ptr(dheads), None, st))
    refused(lib.uav_bc_loss(h, ptr(heads), None, None, n, 5, 1.0 / n, 0.0, 0.0, ptr(sums), ptr(dheads), None, st))
    args = lambda a, n_total, k: (h, ptr(pol.flat), ptr(obs), a, None, n_total, None, 0, k, 1.0 / n, 0.0, 0.0, ptr(sums), ptr(grad), st)
    refused(lib.uav_mlp_bc_grad(*args(ptr(act), n, 3)))
    refused(lib.uav_mlp_bc_grad(*args(ptr(act), 0, 0)))
    refused(lib.uav_mlp_bc_grad(*args(None, n, 0)))
    with pytest.raises(RuntimeError, match="trend_k"):
        ops.mlp_bc_grad(pol.flat, obs, act, None, 1.0 / n, 0.0, 0.0, sums, grad, trend_k=3)


# ---------------------------------------------------------------------------------------------- 7. hand-over
@pytest.fixture(scope="module")
def scripts():
    if PKG not in sys.path:
        sys.path.insert(0, PKG)
    import evaluate_with_lstm
    import generate_expert_data
    import train_bc
    return generate_expert_data, train_bc, evaluate_with_lstm


@pytest.mark.parametrize("kind", ["mlp", "lstm"])
def test_train_bc_checkpoint_loads_and_reports_its_own_accuracy(scripts, kind, tmp_path):
    """Expert data of a hand-made policy P -> train_bc -> the checkpoint through load_policy / load_lstm_policy.  accuracy of
    metrics() after one more epoch at lr = 0 (the parameters no longer move) is the share of expert states on which the loaded
    policy's greedy action is P's: the same number computed two ways, up to samples whose two largest logits are within GAP."""
    ged, train_bc, ev = scripts
    from uavppo import bc
    teacher = towards_mlp(7)
    data = str(tmp_path / "expert.npz")
    states, actions = ged.generate_expert_data(teacher, num_episodes=12, max_steps=40, out=data, lengths=True, seed=5)
    assert sorted(np.load(data).files) == ["actions", "lengths", "states"] and int(np.load(data)["lengths"].sum()) == len(actions)
    out = str(tmp_path / "bc_model.pth")
    tr = train_bc.train_bc(data, kind, hidden=64, layers=1, epochs=3, batch=256 if kind == "mlp" else 5, out=out, lr=3e-3,
                           metrics_path=str(tmp_path / "bc_metrics.csv"))
    rows = open(tmp_path / "bc_metrics.csv").read().strip().split("\n")
    assert rows[0] == "epoch,nll,value_loss,entropy,accuracy,samples" and len(rows) == 4
    tr.lr = 0.0
    before = tr.policy.flat.clone()
    tr.epoch()
    assert torch.equal(before, tr.policy.flat)
    m = tr.metrics()
    assert m["samples"] == len(actions)
    pol = ged.load_policy(out, DEV)
    if kind == "lstm":
        pol2 = ev.load_lstm_policy(out, DEV)
        assert torch.equal(pol2.flat, tr.policy.flat) and torch.equal(pol.flat, pol2.flat)
        s3, a2, _ = bc.load_expert_sequences(data, DEV)
        E, T = a2.shape
        h0, c0 = pol2.zero_state(E)
        logits = pol2.heads(s3, torch.ones(E, T, device=DEV), h0, c0).view(E, T, 6)[..., :5]
        real = a2 >= 0
        logits, want = logits[real], a2[real].long()
    else:
        core = getattr(pol, "core", pol)                     # model.PPOActorCritic keeps its MLPActorCritic as .core
        assert torch.equal(core.flat, tr.policy.flat)
        logits = core.heads(d(states))[:, :5]
        want = d(actions)
    top = logits.topk(2, -1)[0]
    ties = int(((top[:, 0] - top[:, 1]) < GAP).sum())
    agree = int((logits.argmax(-1) == want).sum())
    print(kind, "accuracy", m["accuracy"], agree / len(actions), "near ties", ties)
    assert abs(m["accuracy"] * len(actions) - agree) <= ties
