"""Shuffled env-sequence minibatches: uav_gather_rows_multi against torch.index_select, and VecPPOTrainer(shuffle_envs=True)
-- the identity permutation against the unshuffled trainer bit for bit, forced random permutations against the torch-CPU
oracle update cut the same way, and the permutations the trainer draws by itself."""
import numpy as np
import pytest
import torch

from oracle import ppo_oracle as po

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -7.5


# --------------------------------------------------------------------------------------------- the gather kernel
def _arrays(N, T, D, L, H, seed):
    """The nine arrays a minibatch gathers, as (source, row dimension): act is i32, the rest f32."""
    g = torch.Generator().manual_seed(seed)
    f = lambda *s: torch.randn(*s, generator=g)
    return [(f(N, T, D), 0), (f(N, T), 0), (torch.randint(0, 5, (N, T), generator=g, dtype=torch.int32), 0), (f(N, T), 0),
            (f(N, T), 0), (f(N, T), 0), (f(N, T), 0), (f(L, N, H), 1), (f(L, N, H), 1)]


def _select(N, n_sel, seed):
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(seed))
    assert not torch.equal(perm.sort().values, perm)       # unsorted; n_sel = N: a full permutation, so it holds 0 and N - 1
    return perm[:n_sel]


@pytest.mark.parametrize("N,T,D,L,H,n_sel", [(7, 9, 7, 1, 64, 5),          # rows of 252 B and 36 B: the 4-byte path, shorter than a wave
                                             (12, 128, 8, 2, 256, 1),     # 4 KB rows (several passes of a wave), two planes, one row selected
                                             (33, 16, 6, 2, 128, 33)])    # a full unsorted permutation
def test_gather_rows_multi_equals_index_select(N, T, D, L, H, n_sel):
    from uavppo import ops
    extra = 3
    idx = _select(N, n_sel, seed=N)
    srcs = [(a.to(DEV), rd) for a, rd in _arrays(N, T, D, L, H, seed=N + T)]
    dsts = []
    for a, rd in srcs:
        shape = list(a.shape)
        shape[rd] = n_sel + extra                              # a few rows more than selected: they must keep the sentinel
        dsts.append(torch.full(shape, SENTINEL, dtype=a.dtype, device=DEV))
    ops.gather_rows_multi(idx.to(DEV, torch.int32), [(a, d, rd) for (a, rd), d in zip(srcs, dsts)])
    torch.cuda.synchronize()
    for k, ((a, rd), d) in enumerate(zip(srcs, dsts)):
        want = torch.index_select(a, rd, idx.to(DEV))
        got, rest = d.narrow(rd, 0, n_sel), d.narrow(rd, n_sel, extra)
        assert got.dtype == want.dtype and torch.equal(got, want), (k, tuple(a.shape))
        assert torch.equal(rest, torch.full_like(rest, SENTINEL)), (k, "rows past n_sel were written")


def test_gather_rows_multi_refuses_bad_arguments():
    from uavppo import ops
    idx = torch.arange(2, dtype=torch.int32, device=DEV)
    src, dst = torch.zeros(4, 3, device=DEV), torch.zeros(2, 3, device=DEV)
    with pytest.raises(RuntimeError, match="torch.int32"):
        ops.gather_rows_multi(idx.long(), [(src, dst)])
    with pytest.raises(RuntimeError, match="destinations of 2 rows"):
        ops.gather_rows_multi(torch.arange(3, dtype=torch.int32, device=DEV), [(src, dst)])
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.gather_rows_multi(idx, [(src.t(), dst)])
    with pytest.raises(RuntimeError, match="differ outside the row dimension"):
        ops.gather_rows_multi(idx, [(src, torch.zeros(2, 4, device=DEV))])
    with pytest.raises(RuntimeError, match="expected torch.float32"):
        ops.gather_rows_multi(idx, [(src, dst.to(torch.int32))])
    with pytest.raises(RuntimeError, match="source rows"):
        ops.gather_rows_multi(idx, [(src, dst), (torch.zeros(5, 3, device=DEV), dst.clone())])
    with pytest.raises(RuntimeError, match="multiple of 4"):
        ops.gather_rows_multi(idx, [(torch.zeros(4, 3, dtype=torch.uint8, device=DEV), torch.zeros(2, 3, dtype=torch.uint8, device=DEV))])
    with pytest.raises(RuntimeError, match="13 arrays"):
        ops.gather_rows_multi(idx, [(src, dst.clone()) for _ in range(13)])


# --------------------------------------------------------------------------------------------- the trainer
def cpu_params(policy):
    return {k: v.detach().cpu().clone() for k, v in policy.named_views().items()}


def _fill_synthetic(tr, N, T, seed):
    """Synthetic rollout buffers with done at 8 %, so that restarts (keep = 0) fall inside the gathered sequences."""
    rng = np.random.RandomState(seed)
    d = {"obs": rng.rand(N, T, 6).astype(np.float32), "act": rng.randint(0, 5, (N, T)).astype(np.int32),
         "rew": rng.randn(N, T).astype(np.float32), "val": rng.randn(N, T).astype(np.float32),
         "logp": (np.log(0.2) + 0.1 * rng.randn(N, T)).astype(np.float32),
         "done": (rng.rand(N, T) < 0.08).astype(np.float32)}
    d["keep"] = np.ones((N, T), np.float32)
    d["keep"][:, 1:] = 1 - d["done"][:, :-1]
    last_val = rng.randn(N).astype(np.float32)
    for k, v in d.items():
        tr.buf[k].copy_(torch.from_numpy(v))
    if tr.last_val is not None:
        tr.last_val.copy_(torch.from_numpy(last_val))
    return d, last_val


@pytest.mark.parametrize("policy,H,L,N,T,M", [("lstm", 64, 1, 8, 24, 2), ("lstm", 128, 1, 20, 33, 4), ("lstm", 64, 2, 12, 9, 3),
                                              ("mlp", 0, 0, 8, 32, 2)])
def test_identity_permutation_is_the_unshuffled_update_bit_for_bit(policy, H, L, N, T, M):
    """The packed path runs the same kernels on the same bytes in the same order: with the identity forced as every epoch's
    permutation, parameters, Adam moments and every step's (loss sums, gradient norm) equal the unshuffled trainer's."""
    from uavppo.trainer import VecPPOTrainer
    kw = dict(device=DEV, seed=3, use_curriculum=False, epochs=2, num_minibatches=M, **(dict(hidden=H, layers=L) if policy == "lstm" else {}))
    a, b = VecPPOTrainer(N, T, policy, shuffle_envs=True, **kw), VecPPOTrainer(N, T, policy, **kw)
    start = a.policy.flat.clone()
    assert torch.equal(start, b.policy.flat)
    a.forced_perms = [torch.arange(N) for _ in range(2)]
    g = torch.Generator().manual_seed(N)
    h0, c0 = (torch.randn(L, N, H, generator=g) * 0.3 for _ in range(2)) if policy == "lstm" else (None, None)
    for tr in (a, b):
        _fill_synthetic(tr, N, T, seed=N + M)
        if policy == "lstm":
            tr.h0.copy_(h0)
            tr.c0.copy_(c0)
        tr.record = True
        tr.update()
    torch.cuda.synchronize()
    assert a.forced_perms == [] and len(a.perm_log) == 2 and len(a.log) == len(b.log) == 2 * M
    assert (a.policy.flat - start).abs().max().item() > 1e-5                      # the update moved the parameters
    assert torch.equal(a.policy.flat, b.policy.flat)
    assert torch.equal(a.exp_avg, b.exp_avg) and torch.equal(a.exp_avg_sq, b.exp_avg_sq)
    for i, ((sa, ga), (sb, gb)) in enumerate(zip(a.log, b.log)):
        assert torch.equal(sa, sb) and torch.equal(ga, gb), (i, sa, sb, ga, gb)
    assert a.losses() == b.losses()


def oracle_lstm_update_perms(p, adam, d, h0, c0, perms, M, gae_mode, last_val):
    """tests/test_gpu_trainer.py's oracle_lstm_update (_update_model, train_ppo2.0.py:15-88, torch-CPU autograd) with the
    minibatches of epoch e cut from perms[e]: minibatch m is the whole sequences of envs perms[e][m * nb:(m + 1) * nb], in that
    order, one optimiser step each."""
    rew, val, done = d["rew"], d["val"], d["done"]
    adv = po.gae_reference_exact(rew, val, done) if gae_mode == "reference_exact" else po.gae_standard(rew, val, done, last_val)
    adv, ret = po.normalise(adv, val)
    N, T = rew.shape
    nb = N // M
    x = torch.from_numpy(d["obs"]).transpose(0, 1)
    k = torch.from_numpy(d["keep"]).transpose(0, 1)
    adv2, ret2 = adv.reshape(N, T), ret.reshape(N, T)
    act, logp, val_t = torch.from_numpy(d["act"]), torch.from_numpy(d["logp"]), torch.from_numpy(val)
    log = []
    for perm in perms:
        for m in range(M):
            e = perm[m * nb:(m + 1) * nb]
            leaf = {n: v.detach().clone().requires_grad_(True) for n, v in p.items()}
            probs, value, _, _ = po.lstm_policy_forward(leaf, x[:, e], h0[:, e], c0[:, e], keep=k[:, e])
            probs = probs.transpose(0, 1).reshape(nb * T, -1)
            value = value.transpose(0, 1).reshape(-1)
            total, pl, vl, ent = po.ppo_losses(probs, value, act[e].reshape(-1), logp[e].reshape(-1), adv2[e].reshape(-1),
                                               ret2[e].reshape(-1), val_t[e].reshape(-1))
            total.backward()
            grads = {n: leaf[n].grad for n in p}
            gn = po.clip_grads(grads)
            adam.step(p, grads)
            log.append([float(pl.detach()), float(vl.detach()), float(ent.detach()), gn])
    return np.array(log), adv.numpy()


@pytest.mark.parametrize("mode", ["reference_exact", "standard"])
@pytest.mark.parametrize("H,N,T,M", [(64, 8, 24, 2), (128, 20, 33, 4), (128, 48, 16, 3)])
def test_shuffled_lstm_update_matches_oracle(H, N, T, M, mode):
    """Forced random permutations, another one per epoch, against the oracle update that cuts the same permutations; the
    tolerances are those of test_gpu_trainer.py::test_lstm_minibatched_update_matches_oracle."""
    from uavppo.trainer import VecPPOTrainer
    tr = VecPPOTrainer(N, T, "lstm", hidden=H, device=DEV, seed=3, gae_mode=mode, use_curriculum=False, epochs=2,
                       num_minibatches=M, shuffle_envs=True)
    d, last_val = _fill_synthetic(tr, N, T, seed=N + M)
    assert 0.04 < d["done"].mean() < 0.13 and (d["keep"] == 0).any()
    g = torch.Generator().manual_seed(100 + N)
    perms = [torch.randperm(N, generator=g) for _ in range(2)]
    assert not torch.equal(perms[0], perms[1]) and not torch.equal(perms[0], torch.arange(N))
    tr.forced_perms = [q.clone() for q in perms]
    h0 = torch.randn(1, N, H) * 0.3
    c0 = torch.randn(1, N, H) * 0.3
    tr.h0.copy_(h0)
    tr.c0.copy_(c0)
    p = cpu_params(tr.policy)
    adam = po.AdamState(p)
    tr.record = True
    tr.update()
    log, adv = oracle_lstm_update_perms(p, adam, d, h0, c0, perms, M, mode, last_val)
    assert len(tr.log) == 2 * M and [q.cpu().tolist() for q in tr.perm_log] == [q.tolist() for q in perms]
    assert np.allclose(tr.adv_n.cpu().numpy().reshape(-1), adv, atol=2e-5, rtol=1e-4)
    n = (N // M) * T
    for i, (sums, gn) in enumerate(tr.log):
        s = sums.cpu().numpy()
        print("step", i, "losses", s[:3] / n, "oracle", log[i, :3], "gnorm", gn.item(), "oracle", log[i, 3])
        assert np.allclose(s[:3] / n, log[i, :3], rtol=2e-4, atol=2e-6), (i, s[:3] / n, log[i])
        assert np.isclose(gn.item(), log[i, 3], rtol=2e-3), (i, gn.item(), log[i, 3])
    got = cpu_params(tr.policy)
    for k in p:
        err = (got[k] - p[k]).abs().max().item()
        print(k, "max |param - oracle|", err)
        assert torch.allclose(got[k], p[k], atol=4e-6, rtol=0), (k, err)
    assert np.allclose(tr.losses(), log[-1, :3], rtol=2e-4, atol=2e-6)


def test_drawn_permutations():
    """No forced_perms: every epoch draws a permutation of range(N) from the generator seeded by (seed, rank) -- two epochs
    differ, the same seed repeats the sequence, another rank draws another one."""
    from uavppo.trainer import VecPPOTrainer
    N, T = 64, 4

    def drawn(seed, rank):
        # (rank 1 of 2 without a process group: its all-reduces are no-ops, its generator is rank 1's)
        tr = VecPPOTrainer(N, T, "mlp", device=DEV, seed=seed, rank=rank, world_size=rank + 1, use_curriculum=False, epochs=3,
                           num_minibatches=4, shuffle_envs=True)
        _fill_synthetic(tr, N, T, seed=1)
        tr.record = True
        tr.update()
        assert len(tr.perm_log) == 3 and len(tr.log) == 12
        return [q.cpu() for q in tr.perm_log]

    a, b, c = drawn(5, 0), drawn(5, 0), drawn(5, 1)
    for q in a + c:
        assert q.dtype == torch.int32 and torch.equal(q.sort().values, torch.arange(N, dtype=torch.int32))
    assert not torch.equal(a[0], a[1]) and not torch.equal(a[1], a[2])
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert not any(torch.equal(x, y) for x, y in zip(a, c))
