"""Truncated BPTT (VecPPOTrainer(bptt_len=Lc)): uav_lstm_chunk_states against the torch expression of its definition, the
chunked forward against the full one, the chunked update against a torch-CPU oracle that cuts the same chunk rows, and the
trainer's switches around it (off means off, the identity permutation, a real rollout, truncation semantics)."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import ppo_oracle as po
from test_gpu_env_shuffle import _fill_synthetic, cpu_params

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -7.5


# --------------------------------------------------------------------------------------------- 1. the kernel
def _chunk_states_reference(y, stash, keep, h0, c0, chunk):
    """The definition, in torch on the CPU: row n * C + k = the state carried into step k * chunk, times keep there."""
    N, T, H = y.shape
    Cn = T // chunk
    t0 = torch.arange(Cn) * chunk
    kp = torch.ones(N, Cn) if keep is None else keep[:, t0]
    h, c = torch.empty(N, Cn, H), torch.empty(N, Cn, H)
    h[:, 0], c[:, 0] = h0 * kp[:, 0:1], c0 * kp[:, 0:1]
    h[:, 1:] = y[:, t0[1:] - 1] * kp[:, 1:, None]
    c[:, 1:] = stash[:, t0[1:], 4 * H:5 * H] * kp[:, 1:, None]
    return h.reshape(N * Cn, H), c.reshape(N * Cn, H)


def _chunk_inputs(N, T, H, chunk, seed):
    g = torch.Generator().manual_seed(seed)
    y, stash = torch.randn(N, T, H, generator=g), torch.randn(N, T, 6 * H, generator=g)
    h0, c0 = torch.randn(N, H, generator=g), torch.randn(N, H, generator=g)
    keep = (torch.rand(N, T, generator=g) > 0.3).float()
    keep[::2, ::chunk] = 0.0                   # zeros ON chunk starts (k = 0 included) ...
    keep[1::2, ::chunk] = 1.0                  # ... and ones on them, beside the random zeros elsewhere
    assert (keep[:, ::chunk] == 0).any() and (keep[:, ::chunk] == 1).any()
    assert chunk == 1 or (keep == 0).sum() > (keep[:, ::chunk] == 0).sum()          # (chunk = 1: every step is a chunk start)
    return y, stash, keep, h0, c0


@pytest.mark.parametrize("N,T,chunk,H", [(19, 12, 4, 64), (5, 6, 1, 128), (33, 8, 8, 256), (7, 6, 3, 20)])
def test_chunk_states_equal_the_slices_bit_for_bit(N, T, chunk, H):
    """N = 19 / 33: no multiple of 16; chunk = 1 and chunk = T: every step / only step 0 starts a chunk; H = 20: the 4-byte
    path.  With keep, with keep = NULL, and into an output that is only 4-byte aligned."""
    from uavppo import ops
    y, stash, keep, h0, c0 = _chunk_inputs(N, T, H, chunk, seed=N * T + H)
    dv = [a.to(DEV) for a in (y, stash, keep, h0, c0)]
    rows = N * (T // chunk)
    for kp_cpu, kp in ((keep, dv[2]), (None, None)):
        want_h, want_c = _chunk_states_reference(y, stash, kp_cpu, h0, c0, chunk)
        got_h, got_c = ops.lstm_chunk_states(dv[0], dv[1], kp, dv[3], dv[4], chunk)
        assert got_h.shape == (rows, H) and torch.equal(got_h.cpu(), want_h) and torch.equal(got_c.cpu(), want_c)
        # h_out one float into an allocation: 4-byte aligned only (the scalar path whatever H is); its neighbours stay
        flat = torch.full((rows * H + 2,), SENTINEL, device=DEV)
        view = flat[1:1 + rows * H].view(rows, H)
        assert view.data_ptr() % 16 == 4
        c_out = torch.full((rows + 1, H), SENTINEL, device=DEV)
        ops.lstm_chunk_states(dv[0], dv[1], kp, dv[3], dv[4], chunk, h_out=view, c_out=c_out[:rows])
        assert torch.equal(view.cpu(), want_h) and torch.equal(c_out[:rows].cpu(), want_c)
        assert flat[0].item() == SENTINEL and flat[-1].item() == SENTINEL and bool((c_out[rows] == SENTINEL).all())


def test_chunk_states_refuses_bad_arguments():
    from uavppo import _lib, ops
    lib = _lib.lib()
    N, T, H = 4, 6, 8
    y, stash = torch.zeros(N, T, H, device=DEV), torch.zeros(N, T, 6 * H, device=DEV)
    h0, c0 = torch.zeros(N, H, device=DEV), torch.zeros(N, H, device=DEV)
    ho, co = torch.full((N * T, H), SENTINEL, device=DEV), torch.full((N * T, H), SENTINEL, device=DEV)
    ctx, stream = ops.Context.get(DEV).handle, C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())

    def call(n=N, t=T, h=H, chunk=2, **nulls):
        a = {"y": p(y), "stash": p(stash), "h0": p(h0), "c0": p(c0), "h_out": p(ho), "c_out": p(co)}
        a.update({k: None for k in nulls})
        rc = lib.uav_lstm_chunk_states(ctx, a["y"], a["stash"], None, a["h0"], a["c0"], n, t, h, chunk, a["h_out"], a["c_out"], stream)
        return rc, lib.uav_last_error().decode()

    assert call()[0] == 0
    for kw, reason in [(dict(chunk=0), "chunk=0"), (dict(chunk=-2), "chunk=-2"), (dict(chunk=4), "not a multiple of chunk"),
                       (dict(h=0), "H=0"), (dict(n=1 << 20, t=64, h=64, chunk=8), "below 2^31"),
                       (dict(y=1), "NULL"), (dict(stash=1), "NULL"), (dict(h0=1), "NULL"), (dict(c0=1), "NULL"),
                       (dict(h_out=1), "NULL"), (dict(c_out=1), "NULL")]:
        ho.fill_(SENTINEL)
        rc, err = call(**kw)
        assert rc != 0 and "uav_lstm_chunk_states" in err and reason in err, (kw, rc, err)
        torch.cuda.synchronize()
        assert bool((ho == SENTINEL).all()), kw                  # refused before the launch
    with pytest.raises(RuntimeError, match="not a multiple of chunk"):
        ops.lstm_chunk_states(y, stash, None, h0, c0, 4)


# --------------------------------------------------------------------------------------------- 2. chunked forward = full forward
@pytest.mark.parametrize("H,L,D", [(64, 1, 6), (128, 1, 6), (64, 2, 6), (128, 1, 8), (256, 2, 8)])
def test_chunked_forward_equals_the_full_forward(H, L, D):
    """Every forward form the update can take (the h = 64 / 128 sequence kernels with 6 and with 8 inputs, the generic stacked
    path, the h = 256 step kernels): a step's arithmetic per env depends neither on its tile neighbours nor on its position in
    the sequence, so the heads over the [N * C][Lc] view, started from the extracted states, are the full pass's bit for bit."""
    from uavppo import ops
    from uavppo.policy import LSTMActorCritic
    N, T, Lc = 20, 16, 4
    Cn = T // Lc
    pol = LSTMActorCritic(D, H, L, 5, torch.device(DEV), seed=7)
    g = torch.Generator().manual_seed(H + L + D)
    obs = torch.rand(N, T, D, generator=g).to(DEV)
    keep = (torch.rand(N, T, generator=g) > 0.1).float()
    keep[3, 4] = keep[7, 8] = keep[11, 12] = keep[0, 0] = 0.0          # restarts on chunk starts too
    assert (keep.reshape(N, Cn, Lc)[:, :, 1:] == 0).any()
    keep = keep.to(DEV)
    h0, c0 = (torch.randn(L, N, H, generator=g) * 0.3).to(DEV), (torch.randn(L, N, H, generator=g) * 0.3).to(DEV)
    full = pol.heads(obs, keep, h0, c0).clone()
    h0c, c0c = torch.empty(L, N * Cn, H, device=DEV), torch.empty(L, N * Cn, H, device=DEV)
    for l, (_, stash, y, _) in enumerate(pol._saved[0]):
        ops.lstm_chunk_states(y, stash, keep, h0[l], c0[l], Lc, h0c[l], c0c[l])
    chunked = pol.heads(obs.view(N * Cn, Lc, D), keep.view(N * Cn, Lc), h0c, c0c)
    assert full.shape == chunked.shape == (N * T, 6)
    diff = (full - chunked).abs().max().item()
    print("max |full - chunked|", diff)
    assert torch.equal(full, chunked), diff


# --------------------------------------------------------------------------------------------- 3. the update against the oracle
def _fill(tr, N, T, seed, D=6):
    """test_gpu_env_shuffle.py's _fill_synthetic (done at 8 %); with the trend channels its twin with D features."""
    if D == 6:
        return _fill_synthetic(tr, N, T, seed)
    rng = np.random.RandomState(seed)
    d = {"obs": rng.rand(N, T, D).astype(np.float32), "act": rng.randint(0, 5, (N, T)).astype(np.int32),
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


def oracle_chunked_update(p, adam, d, h0, c0, Lc, perms, M, gae_mode, last_val):
    """_update_model (train_ppo2.0.py:15-88, torch-CPU autograd) under truncated BPTT: the buffer as N * C sequences of Lc steps
    (row n * C + k), each started from the state a no-gradient forward over the steps before it gives at the INITIAL parameters
    (lstm_policy_forward applies keep at the chunk's first step itself); minibatch m of epoch e is the chunk rows
    perms[e][m R:(m + 1) R], one optimiser step each."""
    rew, val, done = d["rew"], d["val"], d["done"]
    adv = po.gae_reference_exact(rew, val, done) if gae_mode == "reference_exact" else po.gae_standard(rew, val, done, last_val)
    adv, ret = po.normalise(adv, val)
    N, T = rew.shape
    Cn, D = T // Lc, d["obs"].shape[2]
    S, R = N * Cn, N * Cn // M
    x = torch.from_numpy(d["obs"]).transpose(0, 1)
    k = torch.from_numpy(d["keep"]).transpose(0, 1)
    hs, cs = [h0], [c0]
    with torch.no_grad():
        for c in range(1, Cn):
            _, _, _, (hn, cn) = po.lstm_policy_forward(p, x[:c * Lc], h0, c0, keep=k[:c * Lc])
            hs.append(hn)
            cs.append(cn)
    h0c = torch.stack(hs, 2).reshape(h0.shape[0], S, -1).clone()         # [L, N, C, H] -> [L, N * C, H]
    c0c = torch.stack(cs, 2).reshape(h0.shape[0], S, -1).clone()
    xc = torch.from_numpy(d["obs"]).reshape(S, Lc, D).transpose(0, 1)
    kc = torch.from_numpy(d["keep"]).reshape(S, Lc).transpose(0, 1)
    rows = lambda a: torch.as_tensor(a).reshape(S, Lc)
    act, logp, val_t, adv2, ret2 = rows(d["act"]), rows(d["logp"]), rows(val), rows(adv), rows(ret)
    log = []
    for perm in perms:
        for m in range(M):
            e = perm[m * R:(m + 1) * R]
            leaf = {n: v.detach().clone().requires_grad_(True) for n, v in p.items()}
            probs, value, _, _ = po.lstm_policy_forward(leaf, xc[:, e], h0c[:, e], c0c[:, e], keep=kc[:, e])
            probs = probs.transpose(0, 1).reshape(R * Lc, -1)
            value = value.transpose(0, 1).reshape(-1)
            total, pl, vl, ent = po.ppo_losses(probs, value, act[e].reshape(-1), logp[e].reshape(-1), adv2[e].reshape(-1),
                                               ret2[e].reshape(-1), val_t[e].reshape(-1))
            total.backward()
            grads = {n: leaf[n].grad for n in p}
            gn = po.clip_grads(grads)
            adam.step(p, grads)
            log.append([float(pl.detach()), float(vl.detach()), float(ent.detach()), gn])
    return np.array(log), adv.numpy()


def _check_against_oracle(H, L, N, T, Lc, M, mode, shuffle, D=6, param_atol=4e-6):
    from uavppo.trainer import VecPPOTrainer
    Cn, epochs = T // Lc, 2
    S = N * Cn
    tr = VecPPOTrainer(N, T, "lstm", hidden=H, layers=L, device=DEV, seed=3, gae_mode=mode, use_curriculum=False, epochs=epochs,
                       num_minibatches=M, shuffle_envs=shuffle, bptt_len=Lc, trend_k=D - 6)
    d, last_val = _fill(tr, N, T, seed=N + M, D=D)
    assert 0.04 < d["done"].mean() < 0.13
    assert (d["keep"].reshape(N, Cn, Lc)[:, 1:, 0] == 0).any()          # a restart really falls on a chunk start
    if shuffle:
        g = torch.Generator().manual_seed(100 + N)
        perms = [torch.randperm(S, generator=g) for _ in range(epochs)]
        assert not torch.equal(perms[0], perms[1]) and not torch.equal(perms[0], torch.arange(S))
        tr.forced_perms = [q.clone() for q in perms]
    else:
        perms = [torch.arange(S) for _ in range(epochs)]
    g = torch.Generator().manual_seed(N)
    h0, c0 = torch.randn(L, N, H, generator=g) * 0.3, torch.randn(L, N, H, generator=g) * 0.3
    tr.h0.copy_(h0)
    tr.c0.copy_(c0)
    p = cpu_params(tr.policy)
    adam = po.AdamState(p)
    tr.record = True
    tr.update()
    log, adv = oracle_chunked_update(p, adam, d, h0, c0, Lc, perms, M, mode, last_val)
    assert len(tr.log) == epochs * M
    if shuffle:
        assert [q.cpu().tolist() for q in tr.perm_log] == [q.tolist() for q in perms]
    assert np.allclose(tr.adv_n.cpu().numpy().reshape(-1), adv, atol=2e-5, rtol=1e-4)
    n = (S // M) * Lc
    for i, (sums, gn) in enumerate(tr.log):
        s = sums.cpu().numpy()
        print("step", i, "losses", s[:3] / n, "oracle", log[i, :3], "gnorm", gn.item(), "oracle", log[i, 3])
        assert np.allclose(s[:3] / n, log[i, :3], rtol=2e-4, atol=2e-6), (i, s[:3] / n, log[i])
        assert np.isclose(gn.item(), log[i, 3], rtol=2e-3), (i, gn.item(), log[i, 3])
    got = cpu_params(tr.policy)
    for k in p:
        err = (got[k] - p[k]).abs().max().item()
        print(k, "max |param - oracle|", err)
        assert torch.allclose(got[k], p[k], atol=param_atol, rtol=0), (k, err)
    assert np.allclose(tr.losses(), log[-1, :3], rtol=2e-4, atol=2e-6)


CASES = [(64, 1, 8, 24, 8, 2), (128, 1, 20, 32, 8, 4), (64, 2, 12, 12, 4, 3)]


@pytest.mark.parametrize("shuffle", [False, True])
@pytest.mark.parametrize("mode", ["reference_exact", "standard"])
@pytest.mark.parametrize("H,L,N,T,Lc,M", CASES)
def test_chunked_lstm_update_matches_oracle(H, L, N, T, Lc, M, mode, shuffle):
    """Tolerances: those of test_gpu_env_shuffle.py::test_shuffled_lstm_update_matches_oracle."""
    _check_against_oracle(H, L, N, T, Lc, M, mode, shuffle)


def test_chunked_h256_stack_update_matches_oracle():
    """h = 256 x 2 with the trend channels (the C5 policy), one minibatch of all 32 chunk rows: the update's forward on the chunk
    view takes the layer-by-layer step path; test_gpu_trainer.py's tolerances for that policy."""
    _check_against_oracle(256, 2, 16, 8, 4, 1, "reference_exact", False, D=8, param_atol=3e-6)


# --------------------------------------------------------------------------------------------- 4. off means off
def test_bptt_len_of_the_whole_horizon_is_the_unchunked_trainer():
    from uavppo.trainer import VecPPOTrainer
    N, T = 32, 16
    kw = dict(hidden=64, device=DEV, seed=11, use_curriculum=False, epochs=2)
    a, b = VecPPOTrainer(N, T, "lstm", bptt_len=T, **kw), VecPPOTrainer(N, T, "lstm", bptt_len=None, **kw)
    for tr in (a, b):
        tr.record = True
        for _ in range(2):
            tr.train_iteration()
    torch.cuda.synchronize()
    assert len(a.log) == len(b.log) == 4
    assert torch.equal(a.policy.flat, b.policy.flat) and torch.equal(a.exp_avg, b.exp_avg) and torch.equal(a.exp_avg_sq, b.exp_avg_sq)
    for (sa, ga), (sb, gb) in zip(a.log, b.log):
        assert torch.equal(sa, sb) and torch.equal(ga, gb)


# --------------------------------------------------------------------------------------------- 5. the identity permutation
@pytest.mark.parametrize("H,L,N,T,Lc,M", CASES)
def test_identity_permutation_is_the_unshuffled_chunked_update_bit_for_bit(H, L, N, T, Lc, M):
    from uavppo.trainer import VecPPOTrainer
    S = N * (T // Lc)
    kw = dict(hidden=H, layers=L, device=DEV, seed=3, use_curriculum=False, epochs=2, num_minibatches=M, bptt_len=Lc)
    a, b = VecPPOTrainer(N, T, "lstm", shuffle_envs=True, **kw), VecPPOTrainer(N, T, "lstm", **kw)
    start = a.policy.flat.clone()
    a.forced_perms = [torch.arange(S) for _ in range(2)]
    g = torch.Generator().manual_seed(N)
    h0, c0 = (torch.randn(L, N, H, generator=g) * 0.3 for _ in range(2))
    for tr in (a, b):
        _fill_synthetic(tr, N, T, seed=N + M)
        tr.h0.copy_(h0)
        tr.c0.copy_(c0)
        tr.record = True
        tr.update()
    torch.cuda.synchronize()
    assert a.forced_perms == [] and len(a.perm_log) == 2 and a.perm_log[0].numel() == S and len(a.log) == len(b.log) == 2 * M
    assert (a.policy.flat - start).abs().max().item() > 1e-5
    assert torch.equal(a.policy.flat, b.policy.flat)
    assert torch.equal(a.exp_avg, b.exp_avg) and torch.equal(a.exp_avg_sq, b.exp_avg_sq)
    for i, ((sa, ga), (sb, gb)) in enumerate(zip(a.log, b.log)):
        assert torch.equal(sa, sb) and torch.equal(ga, gb), (i, sa, sb, ga, gb)
    with pytest.raises(ValueError, match=f"a buffer of {S}"):            # a permutation of the N envs is not one of the chunk rows
        a.forced_perms = [torch.arange(N)]
        a.update()


# --------------------------------------------------------------------------------------------- 6. a real rollout
@pytest.mark.parametrize("reuse", [True, False])
def test_chunked_update_after_a_real_rollout(reuse):
    """Two trainers from one seed collect the same rollout on the fused kernel.  reuse: both adopt the rollout's heads in
    optimiser step 0 (the chunked one through the view, its start states read out of the rollout's own stash), so step 0's loss
    sums are bit-equal.  Without it the chunked trainer runs the state forward and then the chunk rows: item 3's tolerance."""
    from uavppo.trainer import VecPPOTrainer
    N, T, H = 32, 16, 128
    kw = dict(hidden=H, device=DEV, seed=5, use_curriculum=False, epochs=1)
    a, b = VecPPOTrainer(N, T, "lstm", bptt_len=T // 4, **kw), VecPPOTrainer(N, T, "lstm", **kw)
    for tr in (a, b):
        assert tr.rollout_route() == "fused_lstm"
        tr.reuse_rollout_forward = reuse
        tr.record = True
        tr.collect()
        assert tr._rollout_forward_valid is reuse
        tr.update()
    torch.cuda.synchronize()
    for k in a.buf:
        assert torch.equal(a.buf[k], b.buf[k]), k
    sa, sb = a.log[0][0].cpu().numpy(), b.log[0][0].cpu().numpy()
    print("loss sums", sa, sb)
    if reuse:
        assert np.array_equal(sa, sb)
        # the start states of chunk 0 are the rollout's own, and the later ones are not all zero
        assert torch.equal(a.h0c[0].view(N, 4, H)[:, 0], a.h0[0] * a.buf["keep"][:, 0:1]) and a.h0c.abs().max().item() > 0
    else:
        assert np.allclose(sa[:3] / (N * T), sb[:3] / (N * T), rtol=2e-4, atol=2e-6)
    assert not torch.equal(a.policy.flat, b.policy.flat)                  # truncated gradients are other gradients


# --------------------------------------------------------------------------------------------- 7. truncation semantics
@pytest.mark.parametrize("H,L,N,T,Lc", [(64, 1, 8, 24, 8), (128, 1, 20, 32, 8), (64, 2, 12, 12, 4)])
def test_truncated_and_full_bptt_agree_where_every_chunk_start_is_a_restart(H, L, N, T, Lc):
    """With keep = 0 on every chunk start no state and no gradient crosses a chunk boundary in full BPTT either: the two are the
    same function and only the reduction order of the weight gradients differs.  Gradient tolerance: the 2e-3 (relative) of
    test_gpu_trainer.py::test_lstm_ppo_update_matches_oracle, applied to the whole flat gradient."""
    from uavppo.trainer import VecPPOTrainer
    kw = dict(hidden=H, layers=L, device=DEV, seed=3, use_curriculum=False, epochs=2)
    a, b = VecPPOTrainer(N, T, "lstm", bptt_len=Lc, **kw), VecPPOTrainer(N, T, "lstm", **kw)
    assert a.work["y0"].shape == (N * (T // Lc), Lc, H) and b.work["y0"].shape == (N, T, H)      # a really runs on chunk rows
    g = torch.Generator().manual_seed(N)
    h0, c0 = (torch.randn(L, N, H, generator=g) * 0.3 for _ in range(2))
    for tr in (a, b):
        d, _ = _fill_synthetic(tr, N, T, seed=N)
        done = torch.from_numpy(d["done"])
        done[:, Lc - 1::Lc] = 1.0                                           # every chunk's last step ends an episode
        keep = torch.ones(N, T)
        keep[:, 1:] = 1 - done[:, :-1]
        assert bool((keep[:, Lc::Lc] == 0).all())
        tr.buf["done"].copy_(done)
        tr.buf["keep"].copy_(keep)
        tr.h0.copy_(h0)
        tr.c0.copy_(c0)
        tr.record = tr.record_grads = True
        tr.update()
    torch.cuda.synchronize()
    assert len(a.grad_log) == len(b.grad_log) == 2
    for i, ((ga, _), (gb, _)) in enumerate(zip(a.grad_log, b.grad_log)):
        rel = ((ga - gb).norm() / gb.norm()).item()
        print("step", i, "|g_chunked - g_full| / |g_full|", rel)
        assert gb.norm().item() > 0 and rel <= 2e-3, (i, rel)
        assert np.isclose(a.log[i][1].item(), b.log[i][1].item(), rtol=2e-3)
