"""BASELINE.json's full C3 size (4096 envs x 128 steps, LSTM h=128): the benchmarked iteration itself against the
oracle -- rollout rows replayed (test_c3_procedural_rollout_rows_equal_oracle), then GAE, normalisation and the five
optimiser steps of the update on the whole 524,288-sample buffer against the oracle's torch-CPU autograd update
(test_c3_whole_iteration_matches_oracle; the oracle side takes ~10 s of host time) -- plus size-independent properties:
tile independence, linearity of the gradient in the batch, determinism, conservation of the statistics.
Reference: PPOV2.0/train_ppo2.0.py:15-88 (update), :157-198 (rollout).  -m gpu."""
import numpy as np
import pytest
import torch

from oracle import ppo_oracle as po

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, T, H = 4096, 128, 128


@pytest.fixture(scope="module")
def trainer():
    from uavppo.trainer import VecPPOTrainer
    tr = VecPPOTrainer(N, T, "lstm", hidden=H, device=DEV, seed=77, use_curriculum=False)
    tr.collect()
    tr.compute_advantages()
    return tr


def test_gae_and_normalise_fullsize_vs_oracle_rows(trainer):
    b = trainer.buf
    rows = np.random.RandomState(0).choice(N, 24, replace=False)
    rew, val, done = (b[k][rows].cpu().numpy() for k in ("rew", "val", "done"))
    want = po.gae_reference_exact(rew, val, done)
    assert np.allclose(trainer.adv[rows].cpu().numpy(), want, rtol=2e-5, atol=2e-5)
    a = trainer.adv.double()
    s = trainer.stats3.cpu().numpy()
    assert s[2] == N * T and np.isclose(s[0], a.sum().item(), rtol=1e-10)
    an = trainer.adv_n.double()
    assert abs(an.mean().item()) < 1e-5 and abs(an.std().item() - 1.0) < 1e-4          # whole-buffer normalisation
    assert torch.allclose(trainer.ret, trainer.adv_n + b["val"], atol=1e-6)             # returns = normalised adv + V


def test_rollout_fullsize_invariants(trainer):
    b = trainer.buf
    assert torch.isfinite(b["rew"]).all() and torch.isfinite(b["val"]).all() and trainer.nan_count.item() == 0
    assert int(b["act"].min()) >= 0 and int(b["act"].max()) <= 4
    # keep[t] = 1 - done[t-1]; obs[:, :, 4] (step/MAX_STEPS) restarts exactly where an episode ended
    assert torch.equal(b["keep"][:, 1:], 1 - b["done"][:, :-1]) and bool((b["keep"][:, 0] == 1).all())
    step = b["obs"][:, :, 4]
    nxt, ended = step[:, 1:], b["done"][:, :-1] > 0
    assert bool((nxt[ended] == 0).all()) and torch.allclose(nxt[~ended], step[:, :-1][~ended] + 1e-3, atol=1e-6)
    assert torch.allclose(b["logp"].exp().mean(), torch.tensor(0.2, device=DEV), atol=5e-3)   # near-uniform init policy
    # the stash emitted by the rollout is the forward pass of the same parameters
    from uavppo import ops
    v = trainer.policy.views
    y, _, _, _ = ops.lstm_fwd(b["obs"][:64].contiguous(), b["keep"][:64].contiguous(), trainer.h0[0][:64].contiguous(),
                              trainer.c0[0][:64].contiguous(), v["lstm.weight_ih_l0"], v["lstm.weight_hh_l0"],
                              v["lstm.bias_ih_l0"], v["lstm.bias_hh_l0"])
    assert torch.allclose(trainer.work["y0"][:64], y, atol=3e-6)


def test_lstm_fullsize_tile_independence_and_gradient_linearity(trainer):
    """Env tiles are independent problems: a 32-env slice computed alone equals the same slice of the full
    launch bit for bit; and the weight gradient of the full batch is the sum of the gradients of its halves."""
    from uavppo import ops
    b, v = trainer.buf, trainer.policy.views
    w = (v["lstm.weight_ih_l0"], v["lstm.weight_hh_l0"], v["lstm.bias_ih_l0"], v["lstm.bias_hh_l0"])
    h0, c0 = trainer.h0[0], trainer.c0[0]
    y, hn, cn, stash = ops.lstm_fwd(b["obs"], b["keep"], h0, c0, *w)
    sl = slice(1024, 1056)
    y2, hn2, cn2, stash2 = ops.lstm_fwd(b["obs"][sl].contiguous(), b["keep"][sl].contiguous(), h0[sl].contiguous(),
                                        c0[sl].contiguous(), *w)
    assert torch.equal(y[sl], y2) and torch.equal(cn[sl], cn2) and torch.equal(stash[sl][..., :5 * H], stash2[..., :5 * H])
    dheads = torch.randn(N, T, 6, device=DEV, generator=torch.Generator(DEV).manual_seed(4)) / (N * T)
    full = ops.lstm_bwd(b["obs"], b["keep"], stash, w[0], w[1], y, h0, dheads=dheads, w_head=v["head.weight"])
    parts = []
    for lo, hi in ((0, N // 2), (N // 2, N)):
        p = ops.lstm_bwd(b["obs"][lo:hi].contiguous(), b["keep"][lo:hi].contiguous(), stash[lo:hi].contiguous(), w[0], w[1],
                         y[lo:hi].contiguous(), h0[lo:hi].contiguous(), dheads=dheads[lo:hi].contiguous(),
                         w_head=v["head.weight"])
        parts.append(p)
        assert torch.equal(p["dh0"], full["dh0"][lo:hi])
    for k in ("dw_hh", "dw_ih", "db", "dw_head"):
        tot = parts[0][k] + parts[1][k]
        scale = full[k].abs().max().item()
        # f32 sums of 524288 random-sign terms in two groupings: measured residual 5e-7 .. 2.5e-5 of the largest entry over seeds
        assert (full[k] - tot).abs().max().item() <= 1e-4 * scale, k


def test_update_fullsize_is_deterministic_and_finite():
    from uavppo.trainer import VecPPOTrainer
    outs = []
    for _ in range(2):
        tr = VecPPOTrainer(N, T, "lstm", hidden=H, device=DEV, seed=5, use_curriculum=False, epochs=2)
        tr.train_iteration()
        outs.append((tr.policy.flat.clone(), tr.loss_sums.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])     # no atomics: bitwise repeatable
    pl, vl, ent = (outs[0][1][:3] / (N * T)).tolist()
    assert np.isfinite([pl, vl, ent]).all() and 1.55 < ent < 1.6095


def test_lstm_fullsize_scaling_causality_and_heads(trainer):
    """More properties that need no oracle at full size: (a) the backward pass and the weight gradients are linear in
    dheads, and scaling by a power of two is exact in f32 AND commutes with the bf16 operand split, so the results
    must scale bit for bit; (b) the sequence is causal: changing observations from step t0 on leaves y[:, :t0]
    bitwise unchanged; (c) the heads the forward kernel writes are y W_head^T + b_head."""
    from uavppo import ops
    b, v = trainer.buf, trainer.policy.views
    w = (v["lstm.weight_ih_l0"], v["lstm.weight_hh_l0"], v["lstm.bias_ih_l0"], v["lstm.bias_hh_l0"])
    h0, c0 = trainer.h0[0], trainer.c0[0]
    heads = torch.empty(N, T, 6, device=DEV)
    y, hn, cn, stash = ops.lstm_fwd(b["obs"], b["keep"], h0, c0, *w, w_head=v["head.weight"], b_head=v["head.bias"], heads=heads)
    rows = torch.from_numpy(np.random.RandomState(1).choice(N, 40, replace=False)).to(DEV)
    want = y[rows].double() @ v["head.weight"].double().T + v["head.bias"].double()
    assert torch.allclose(heads[rows].double(), want, rtol=1e-5, atol=2e-6)
    # (a)
    g = torch.Generator(device=DEV).manual_seed(3)
    dheads = torch.randn(N, T, 6, generator=g, device=DEV) / (N * T)
    r1 = ops.lstm_bwd(b["obs"], b["keep"], stash, w[0], w[1], y, h0, dheads=dheads, w_head=v["head.weight"])
    keep1 = {k: r1[k].clone() for k in ("dw_hh", "dw_ih", "db", "dw_head", "dh0", "dc0")}
    r4 = ops.lstm_bwd(b["obs"], b["keep"], stash, w[0], w[1], y, h0, dheads=dheads * 4.0, w_head=v["head.weight"])
    for k, t in keep1.items():
        assert torch.equal(r4[k], t * 4.0), k
    # (b)
    t0 = 77
    obs2 = b["obs"].clone()
    obs2[:, t0:] = torch.rand_like(obs2[:, t0:])
    y2, _, _, _ = ops.lstm_fwd(obs2, b["keep"], h0, c0, *w, want_stash=False)
    assert torch.equal(y2[:, :t0], y[:, :t0]) and not torch.equal(y2[:, t0:], y[:, t0:])


def test_fullsize_gradient_split_modes_equal_exact_f32_kernels(trainer):
    """At the full C3 size the whole-batch PPO gradient computed by the kernels of each split arithmetic -- `fp16x3`, the
    default (two fp16 pieces per f32 operand, three products), and `bf16x6`, the one the trainer's range guard switches to
    (three bf16 pieces, six products) -- equals the one from the exact-f32-MFMA kernels to f32 summation noise: the claim
    `dtype: f32` of the bench line, in both modes."""
    from uavppo import ops
    b, pol = trainer.buf, trainer.policy
    n = N * T
    args = (b["act"].reshape(-1), b["logp"].reshape(-1), trainer.adv_n.reshape(-1), trainer.ret.reshape(-1),
            b["val"].reshape(-1), 1.0 / n, 0.2, 0.01)
    grads, sums = {}, {}
    for mode in ("fp16x3", "bf16x6", "f32_mfma"):
        ops.set_lstm_arith(mode)
        heads = pol.heads(b["obs"], b["keep"], trainer.h0, trainer.c0, trainer.work)
        loss = torch.zeros(4, dtype=torch.float64, device=DEV)
        dheads = torch.empty(n, 6, device=DEV)
        dbias = torch.empty(6, device=DEV)
        ops.ppo_loss_heads(heads, *args, loss, dheads, dbias)
        g = pol.backward(dheads, trainer.work, dbias).clone()
        grads[mode] = g.double()
        sums[mode] = loss.clone()
    ops.set_lstm_arith("fp16x3")
    for split in ("fp16x3", "bf16x6"):
        rel = (grads[split] - grads["f32_mfma"]).norm() / grads["f32_mfma"].norm()
        assert rel.item() < 2e-5, (split, rel.item())
        assert torch.allclose(sums[split][1:3], sums["f32_mfma"][1:3], rtol=1e-6), split    # value-loss and entropy sums
        assert abs((sums[split][0] - sums["f32_mfma"][0]).item()) < 1e-4, split             # policy-loss sum: ~0 at init


@pytest.mark.parametrize("radius", [50.0, 140.0])
def test_c3_procedural_rollout_rows_equal_oracle(radius):
    """The benchmarked kernel in the benchmarked mode: rollout_lstm_kernel<128> at C3's exact shape (4096 x 128, h=128,
    procedural field, own noise, own sampled actions).  Oracle replay of env rows chosen over the whole launch -- the
    first and last rows, rows of other workgroups / XCDs, and rows in which an episode ENDS (so the restart, the
    episode-1 field and source, and the keep mask are exercised): every observation / done / keep / flag bit for bit,
    rewards to 1e-6, the sampled action == the inverse-CDF draw of the recorded logits at the oracle's Philox uniform,
    values / log-probs against the f32 oracle LSTM on the recorded observations (rows are independent problems).
    radius 50 is bench.py's start state (episodes rarely end inside 128 steps); radius 140 makes many rows end."""
    from oracle import procedural_oracle as pr
    from uavppo.trainer import VecPPOTrainer
    seed = 1234                                                  # bench.py's seed
    tr = VecPPOTrainer(N, T, "lstm", hidden=H, device=DEV, seed=seed, use_curriculum=False)
    tr.radius = radius
    tr.reset()
    obs0 = tr.cur_obs.cpu().numpy().copy()
    h0, c0 = tr.h.cpu().clone(), tr.c.cpu().clone()
    tr.collect()
    b = {k: v.cpu().numpy() for k, v in tr.buf.items()}
    heads = tr.work["heads"].cpu().numpy()
    ended = np.flatnonzero(b["done"].sum(1) > 0)
    rows = [0, 15, 16, 2047, N - 17, N - 1] + [int(r) for r in ended[:: max(1, len(ended) // 6)][:6]]
    if radius > 100:
        assert len(ended) >= 50, len(ended)
    rows = sorted(set(rows))
    assert len(rows) >= 8
    p = {k: v.detach().cpu().clone() for k, v in tr.policy.named_views().items()}
    n_end = 0
    for r in rows:
        ora = pr.ProceduralVecEnv(1, seed, "v2.0", radius=radius, env_offset=r)
        obs = ora.reset()
        assert np.array_equal(obs0[r:r + 1], obs), r
        keep = np.ones(1, np.float32)
        for t in range(T):
            assert np.array_equal(b["obs"][r:r + 1, t], obs), (r, t)
            assert b["keep"][r, t] == keep[0], (r, t)
            obs, rew, done, reached, _, _ = ora.step(b["act"][r:r + 1, t])
            assert abs(float(b["rew"][r, t]) - float(np.float32(rew[0]))) <= 1e-6, (r, t)
            assert bool(b["done"][r, t] > 0) == bool(done[0]), (r, t)
            assert int(b["flags"][r, t]) == int(done[0]) | (int(reached[0]) << 1), (r, t)
            keep = 1.0 - done.astype(np.float32)
            n_end += int(done[0])
        assert np.array_equal(tr.cur_obs[r:r + 1].cpu().numpy(), obs), r
    # the Categorical draw of those rows
    sel = np.asarray(rows)
    logits = heads[sel][..., :5].astype(np.float32)
    e = np.exp(logits - logits.max(-1, keepdims=True), dtype=np.float32)
    pdev = e / e.sum(-1, keepdims=True, dtype=np.float32)
    u = np.stack([pr.action_uniform(seed, t, sel, 0) for t in range(T)], axis=1)
    cdf = np.cumsum(pdev, -1, dtype=np.float32)
    clear = np.all(np.abs(cdf - (u * cdf[..., -1])[..., None]) > 2e-6, axis=-1)
    want = pr.sample_inverse_cdf(pdev.reshape(-1, 5), u.reshape(-1)).reshape(len(rows), T)
    assert clear.mean() > 0.99 and np.array_equal(want[clear], b["act"][sel][clear])
    # policy side of those rows on the recorded inputs: f32 oracle LSTM (torch CPU)
    with torch.no_grad():
        probs, value, _, _ = po.lstm_policy_forward(p, torch.from_numpy(b["obs"][sel]).transpose(0, 1), h0[:, sel], c0[:, sel],
                                                    keep=torch.from_numpy(b["keep"][sel]).transpose(0, 1))
        lp = po.categorical_logp(probs.transpose(0, 1).reshape(len(rows) * T, -1), torch.from_numpy(b["act"][sel]).reshape(-1).long())
    assert np.allclose(b["val"][sel], value.transpose(0, 1).numpy().reshape(len(rows), T), atol=2e-5, rtol=1e-4)
    assert np.allclose(b["logp"][sel], lp.numpy().reshape(len(rows), T), atol=2e-5, rtol=1e-4)
    assert np.allclose(pdev, probs.transpose(0, 1).numpy(), atol=2e-6)
    if radius > 100:
        assert n_end >= 6
    print(f"C3 procedural replay: rows {rows}, episode ends replayed {n_end}, rows with ends in the launch {len(ended)}")


def test_c3_whole_iteration_matches_oracle():
    """The iteration bench.py times, at its exact shape and seed (4096 x 128, h = 128, procedural field, radius 50, own
    actions, own noise): after the fused rollout, the update on the rollout's own buffers -- epoch 0 adopting the rollout
    kernel's forward pass, epochs 1-4 through lstm_fwd_h3_kernel, five lstm_bwd_h3k_kernel / lstm_wgrad_h3_kernel launches,
    clip + Adam -- against the oracle update (PPOV2.0/train_ppo2.0.py:15-88 semantics, torch-CPU autograd) of the same
    buffers: advantages / returns, per-epoch losses, per-epoch UNclipped gradients, gradient norms, final parameters."""
    from _iteration_check import update_vs_oracle
    from uavppo.trainer import VecPPOTrainer
    tr = VecPPOTrainer(N, T, "lstm", hidden=H, device=DEV, seed=1234, use_curriculum=False)
    tr.collect()
    assert tr._rollout_forward_valid                    # epoch 0 will adopt the rollout's stash, as in the bench
    m = update_vs_oracle(tr, "c3")
    assert m["samples"] == 524288 and len(m["steps"]) == 5


def test_c3_minibatched_iteration_matches_oracle():
    """U1 at full size (train_ppo2.0.py:43-53 with M = 8): the same 4096 x 128 buffers updated in eight minibatches of 512 whole env
    sequences per epoch (no rollout-forward reuse, minibatch-sized work buffers, h0 / c0 slices, loss mean over the minibatch) for two
    epochs = 16 optimiser steps, against the oracle update that slices the same way -- every step's gradient at the same parameters,
    clip + Adam on the same gradients, the free-running loss curve."""
    from _iteration_check import update_vs_oracle
    from uavppo.trainer import VecPPOTrainer
    tr = VecPPOTrainer(N, T, "lstm", hidden=H, device=DEV, seed=4321, use_curriculum=False, num_minibatches=8, epochs=2)
    tr.radius = 120.0                                   # episodes end inside the rollout: restarts in most minibatches
    tr.reset()
    tr.collect()
    assert not tr._rollout_forward_valid
    m = update_vs_oracle(tr, "c3_m8")
    assert len(m["steps"]) == 16 and m["episode_ends"] >= 500
