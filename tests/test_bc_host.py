"""Behaviour cloning, host side (no GPU): the additive signatures, expert episodes cut into padded sequences and back, and the
f64 statement of the cloning loss (bc_oracle, which tests/test_gpu_bc.py leans on) against its own closed-form gradient."""
import inspect
import os
import sys

import numpy as np
import pytest
import torch

from conftest import PKG

F32_EPS = float(np.finfo(np.float32).eps)


def bc_oracle(logits, value, act, vtarget, value_coef, ent_beta):
    """The loss of csrc/loss_core.h: bc_sample over a batch, in the dtype of `logits` (f64 here): returns total and the sums
    (nll, 0.5 (V - R)^2, entropy, agreement count, unmasked count).  act outside 0 .. A-1 masks a row; vtarget None: no value
    term.  Categorical(probs) as oracle/ppo_oracle.py:categorical_logp: renormalise, clamp to [eps, 1 - eps], log."""
    A = logits.shape[-1]
    act = act.long()
    valid = (act >= 0) & (act < A)
    a = act.clamp(0, A - 1)
    p = torch.softmax(logits, -1)
    q = p / p.sum(-1, keepdim=True)
    qa = q.gather(-1, a[:, None])[:, 0].clamp(min=F32_EPS, max=1 - F32_EPS)
    w = valid.to(logits.dtype)
    nll = (-torch.log(qa) * w).sum()
    ent = (-(p * torch.log(p + 1e-8)).sum(-1) * w).sum()
    vl = (0.5 * (value - vtarget) ** 2 * w).sum() if vtarget is not None else torch.zeros((), dtype=logits.dtype)
    n = w.sum().clamp(min=1)
    agree = ((logits.argmax(-1) == a) & valid).sum()
    total = nll / n + value_coef * vl / n - ent_beta * ent / n
    return total, (nll, vl, ent, agree, valid.sum())


def bc_closed_form(logits, value, act, vtarget, value_coef, ent_beta):
    """dz, dV of the issue's per-sample rule, f64, with inv_n = 1 / (unmasked samples)."""
    A = logits.shape[-1]
    act = act.long()
    valid = (act >= 0) & (act < A)
    inv_n = 1.0 / max(int(valid.sum()), 1)
    a = act.clamp(0, A - 1)
    p = torch.softmax(logits, -1)
    q = p / p.sum(-1, keepdim=True)
    qa = q.gather(-1, a[:, None])[:, 0]
    open_ = (qa >= F32_EPS) & (qa <= 1 - F32_EPS)
    g_logp = open_.to(logits.dtype) * -inv_n
    lg = torch.log(p + 1e-8)
    hk = -lg - p / (p + 1e-8)
    ph = (p * hk).sum(-1, keepdim=True)
    onehot = torch.nn.functional.one_hot(a, A).to(logits.dtype)
    dz = g_logp[:, None] * (onehot - q) - ent_beta * inv_n * p * (hk - ph)
    dV = value_coef * inv_n * (value - vtarget) if vtarget is not None else torch.zeros_like(value)
    m = valid.to(logits.dtype)
    return dz * m[:, None], dV * m


@pytest.fixture(scope="module")
def mods():
    if PKG not in sys.path:
        sys.path.insert(0, PKG)
    import generate_expert_data as ged
    from uavppo import bc
    return ged, bc


def test_additive_signatures(mods):
    ged, bc = mods
    import train_ppo_gail
    sig = inspect.signature(ged.generate_expert_data)
    assert sig.parameters["lengths"].default is False
    assert inspect.signature(train_ppo_gail.train_ppo_gail).parameters["init_model"].default is None
    ps = inspect.signature(bc.BCTrainer.__init__).parameters
    assert list(ps)[:3] == ["self", "policy", "expert"]
    want = dict(batch=4096, lr=3e-4, value_coef=0.0, ent_beta=0.0, max_grad_norm=0.5, seed=0, value_targets=None, rank=0, world_size=1)
    assert {k: ps[k].default for k in want} == want
    assert all(ps[k].kind is inspect.Parameter.KEYWORD_ONLY for k in want)
    import config
    assert (config.BC_EPOCHS, config.BC_BATCH, config.BC_LR, config.BC_VALUE_COEF) == (10, 4096, 3e-4, 0.0)
    import train_bc
    assert list(inspect.signature(train_bc.train_bc).parameters)[:7] == ["expert_path", "policy", "hidden", "layers", "epochs", "batch", "out"]


def _records():
    """Four envs, five slots: an episode of length 1, one that fills every slot, one of 3, one of 2 -- 'not stepped' slots
    carry act -1 and the flag bit 2, in two chunks of 2 + 3 steps."""
    rng = np.random.RandomState(0)
    N, S, D = 4, 5, 6
    lens = np.array([1, 5, 3, 2])
    cur = rng.rand(N, D).astype(np.float32)
    obs = rng.rand(N, S, D).astype(np.float32)
    act = rng.randint(0, 5, (N, S)).astype(np.int32)
    flags = np.zeros((N, S), np.uint8)
    for e, n in enumerate(lens):
        flags[e, n - 1] |= 1
        flags[e, n:] = 4
        act[e, n:] = -1
    cut = lambda x: [x[:, :2], x[:, 2:]]
    return cur, obs, act, flags, lens, cut


def test_lengths_pairs_and_sequences_round_trip(mods, tmp_path):
    ged, bc = mods
    cur, obs, act, flags, lens, cut = _records()
    states, actions = ged.expert_pairs(cur, cut(obs), cut(act), cut(flags))
    got = ged.expert_lengths(cut(flags))
    assert got.dtype == np.int64 and np.array_equal(got, lens) and np.array_equal(ged.expert_lengths(flags), lens)
    assert len(actions) == lens.sum()
    s3, a2, ln = bc.load_expert_sequences((states, actions, got), "cpu")
    assert s3.shape == (4, 5, 6) and a2.shape == (4, 5) and a2.dtype == torch.int32 and np.array_equal(ln.numpy(), lens)
    acted_on = np.concatenate([cur[:, None], obs[:, :-1]], 1)
    for e, n in enumerate(lens):
        assert np.array_equal(s3[e, :n].numpy(), acted_on[e, :n]) and np.array_equal(a2[e, :n].numpy(), act[e, :n])
        assert (a2[e, n:] == -1).all() and (s3[e, n:] == 0).all()
    # through a file, and the file without lengths
    p = tmp_path / "e.npz"
    np.savez(p, states=states, actions=actions, lengths=got)
    s3b, a2b, _ = bc.load_expert_sequences(str(p), "cpu")
    assert torch.equal(s3b, s3) and torch.equal(a2b, a2)
    np.savez(p, states=states, actions=actions)
    with pytest.raises(RuntimeError, match="lengths"):
        bc.load_expert_sequences(str(p), "cpu")
    with pytest.raises(RuntimeError, match="lengths"):
        bc.load_expert_sequences((states, actions), "cpu")
    for bad in (lens + np.array([0, 0, 1, 0]), lens[:3]):
        with pytest.raises(RuntimeError, match="summing"):
            bc.load_expert_sequences((states, actions, bad), "cpu")


def test_default_file_has_the_reference_keys(mods, tmp_path, monkeypatch):
    """generate_expert_data's own writing code, with the GPU parts stood in for by the hand-made records."""
    ged, _ = mods
    cur, obs, act, flags, lens, cut = _records()

    class Core:
        obs_dim, device = 6, "cpu"
    monkeypatch.setattr(ged, "policy_core", lambda p: ("lstm", Core()))
    monkeypatch.setattr(ged, "VecMethaneEnv", lambda *a, **k: None)
    monkeypatch.setattr(ged, "greedy_records", lambda *a, **k: (cur, cut(obs), cut(act), cut(flags)))
    out = tmp_path / "d.npz"
    ged.generate_expert_data(object(), 4, out=str(out))
    assert sorted(np.load(out).files) == ["actions", "states"]
    ged.generate_expert_data(object(), 4, out=str(out), lengths=True)
    d = np.load(out)
    assert sorted(d.files) == ["actions", "lengths", "states"] and np.array_equal(d["lengths"], lens) and d["lengths"].dtype == np.int64


@pytest.mark.parametrize("with_vt,vcoef,beta", [(False, 0.0, 0.0), (True, 0.5, 0.01), (False, 0.5, 0.01), (True, 0.0, 0.0)])
def test_f64_oracle_agrees_with_its_closed_form_gradient(with_vt, vcoef, beta):
    g = torch.Generator().manual_seed(5)
    n = 64
    logits = (torch.randn(n, 5, generator=g, dtype=torch.float64) * 4).requires_grad_(True)
    value = torch.randn(n, generator=g, dtype=torch.float64).requires_grad_(True)
    act = torch.randint(0, 5, (n,), generator=g)
    act[::3] = -1
    act[1] = 5
    with torch.no_grad():
        logits[2] = torch.tensor([40.0, 0, 0, 0, 0], dtype=torch.float64)      # q[a] < eps: the clamp binds, no policy gradient
    act[2] = 3
    vt = torch.randn(n, generator=g, dtype=torch.float64) if with_vt else None
    total, sums = bc_oracle(logits, value, act, vt, vcoef, beta)
    total.backward()
    dz, dV = bc_closed_form(logits.detach(), value.detach(), act, vt, vcoef, beta)
    assert int(sums[4]) == n - len(range(0, n, 3)) - 1
    assert torch.allclose(logits.grad, dz, rtol=1e-9, atol=1e-14), (logits.grad - dz).abs().max()
    assert torch.allclose(value.grad if value.grad is not None else torch.zeros(n, dtype=torch.float64), dV, rtol=1e-12, atol=0)
    assert (dz[::3] == 0).all() and (dz[1] == 0).all()
    if beta == 0:
        assert (dz[2] == 0).all()
    assert (dz[4] != 0).all()
