"""BASELINE.json's OTHER configurations at their exact per-GPU shapes (C3 is tests/test_gpu_fullsize.py):

  C2  256 envs x 64 steps, LSTM h=64                      whole iteration against the oracle (16,384 samples: CPU seconds)
  C4  1024 envs x 128 steps per GPU, h=128, PPOV2.1 (sigma 15), materialised bank of F=64 fields built by
      uav_env_materialise, through rollout_lstm_kernel    oracle rows + invariants + whole iteration against the oracle
  C5  4096 envs x 256 steps per GPU, h=256 x 2, obs 6+2   tile independence, determinism, fp16-split vs exact-f32
      gradient, pipelined vs per-layer backward bit-equality -- properties at 1 M samples; ONE step-kernel tile of it
      (64 envs x 256 steps, the same kernels) whole iteration against the oracle; at the full shape, the first optimiser
      step's gradient -- whole batch, every aligned 256-env chunk, two unaligned env sets -- against an f64 oracle streamed
      over env chunks, and the update's own first gradient bit-equal to it

Reference shapes: PPOV2.1/environment.py:52-69 (sigma = 15 field), nn.LSTM stack PPOV2.0/model.py:206-212,
update loop PPOV2.0/train_ppo2.0.py:15-88.  -m gpu."""
import numpy as np
import pytest
import torch

from oracle import ppo_oracle as po
from oracle import procedural_oracle as pr
from oracle.env_oracle import EnvCore

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def cpu_params(policy):
    return {k: v.detach().cpu().clone() for k, v in policy.named_views().items()}


# ------------------------------------------------------------------------------------------------------------ C2
def test_c2_whole_iteration_matches_oracle():
    """One full iteration at C2's exact shape: procedural rollout (own actions, own noise) replayed by the oracle, then
    GAE + normalise + 5 full-batch epochs against the oracle's torch-autograd update on the GPU's buffers: per-epoch
    losses, clipped gradient norms and the parameters after the fifth Adam step."""
    from uavppo.trainer import VecPPOTrainer
    from test_gpu_procedural import _check_rollout_against_oracle
    from test_gpu_trainer import oracle_lstm_update
    N, T, H, seed = 256, 64, 64, 2025
    tr = VecPPOTrainer(N, T, "lstm", hidden=H, variant="v2.0", device=DEV, seed=seed, use_curriculum=False)
    tr.radius = 120.0
    tr.reset()
    ora = pr.ProceduralVecEnv(N, seed, "v2.0", radius=120.0)
    obs0 = ora.reset()
    p = cpu_params(tr.policy)
    adam = po.AdamState(p)
    h0, c0 = tr.h.cpu().clone(), tr.c.cpu().clone()
    tr.collect()
    b = {k: v.cpu().numpy() for k, v in tr.buf.items()}
    assert _check_rollout_against_oracle(tr, ora, obs0, b) >= 10          # episodes end inside the rollout
    tr.record = True
    tr.update()
    log, adv_n, ret = oracle_lstm_update(p, adam, b["obs"], b["act"], b["rew"], b["val"], b["logp"], b["done"], b["keep"],
                                         h0, c0, tr.hp["epochs"], "reference_exact", None)
    assert np.allclose(tr.adv_n.cpu().numpy().reshape(-1), adv_n, atol=3e-5, rtol=1e-4)
    assert np.allclose(tr.ret.cpu().numpy().reshape(-1), ret, atol=3e-5, rtol=1e-4)
    assert len(tr.log) == 5
    for e, (sums, gn) in enumerate(tr.log):
        got = sums.cpu().numpy()[:3] / (N * T)
        assert np.allclose(got, log[e, :3], rtol=2e-4, atol=2e-6), (e, got, log[e])
        assert np.isclose(gn.item(), log[e, 3], rtol=2e-3), (e, gn.item(), log[e, 3])
    # parameters after the fifth Adam step of the reference's lr (3e-5): the bar of the small-shape update tests
    # (tests/test_gpu_trainer.py: 3e-6 = a tenth of one step) -- Adam turns a gradient element's relative error into
    # lr x that error, and elements that nearly cancel over 16,384 samples carry the largest
    # A few elements are exempt by construction: where the gradient cancels to rounding noise -- the critic bias at epoch 0
    # is sum(V - ret) = -sum(adv_n) = 0 by the normalisation itself -- Adam's step is lr * sign(noise); such an element
    # may differ by up to 2 * epochs * lr.
    got = cpu_params(tr.policy)
    n_far = n_all = 0
    for k in p:
        d = (got[k] - p[k]).abs()
        n_far += int((d > 3e-6).sum())
        n_all += d.numel()
        assert d.max().item() <= 2 * 5 * 3e-5, (k, d.max().item())
    assert n_far <= 1e-3 * n_all + 2, (n_far, n_all)


# ------------------------------------------------------------------------------------------------------------ C4
@pytest.fixture(scope="module")
def c4():
    """C4's per-GPU trainer exactly as bench.py builds it: bank of 64 sigma=15 fields from uav_env_materialise."""
    from uavppo import ops
    from uavppo.trainer import VecPPOTrainer
    from uavppo.vec_env import VecMethaneEnv
    F, N, T = 64, 1024, 128
    gen = VecMethaneEnv(F, "v2.1", DEV, seed=4321)
    gen.reset()
    bank = torch.stack([ops.env_materialise(gen.state, F, gen.cfg(), f) for f in range(F)])
    src = gen.peek()[1]
    tr = VecPPOTrainer(N, T, "lstm", hidden=128, variant="v2.1", device=DEV, seed=1234, bank=bank, bank_sources=src,
                       use_curriculum=False)
    tr.radius = 90.0
    tr.reset()
    obs0 = tr.cur_obs.cpu().numpy().copy()
    tr.collect()
    return tr, bank.cpu().numpy(), src.cpu().numpy(), obs0


def test_c4_bank_is_the_sigma15_field(c4):
    """The bank bench.py's C4 uses IS E3 with sigma = 15 (PPOV2.1/environment.py:56): cell for cell against the oracle."""
    _, bank, src, _ = c4
    for f in (0, 17, 63):
        want_src, conc, tke = pr.full_field(4321, f, 0, 15.0)
        assert np.array_equal(src[f], want_src)
        assert np.abs(bank[f, ..., 0] - conc).max() <= 1e-11 and np.abs(bank[f, ..., 1] - tke).max() <= 1e-11
    # a sigma = 15 plume is narrow: 100 ppm at the source, below 1 + turbulence 60 cells away
    f = 5
    sx, sy = int(src[f, 0]), int(src[f, 1])
    assert bank[f, sx, sy, 0] == 100.0 and bank[f, min(sx + 60, 499), sy, 0] < 20.0


def test_c4_rollout_rows_equal_oracle(c4):
    """rollout_lstm_kernel with variant v2.1 over the materialised bank at 1024 x 128: 16 env rows (first, last, and
    rows whose episodes ended) replayed by the oracle from the bank tables -- field choice (env + episode * N) mod F,
    the counter RNG's step noise -- bit for bit; whole-buffer invariants."""
    tr, bank, src, obs0 = c4
    N, T, F = tr.N, tr.T, bank.shape[0]
    b = {k: v.cpu().numpy() for k, v in tr.buf.items()}
    ended = np.nonzero(b["done"].sum(1) > 0)[0]
    assert len(ended) >= 8
    rows = sorted(set([0, 1, 15, 16, N - 1] + ended[:11].tolist()))
    for i in rows:
        e = EnvCore("v2.1")
        e.radius = 90.0
        episode = 0

        def begin():
            f = (i + episode * N) % F
            return e.begin_episode(src[f], bank[f, ..., 0], bank[f, ..., 1])

        o = begin()
        assert np.array_equal(o, obs0[i])
        for t in range(T):
            assert np.array_equal(b["obs"][i, t], o), (i, t)
            z = pr.step_normals(1234, i, episode, e.steps)
            o, r, d, reached, _ = e.step(int(b["act"][i, t]), z)
            assert abs(b["rew"][i, t] - np.float32(r)) <= 1e-6 and bool(b["done"][i, t]) == d, (i, t)
            assert int(b["flags"][i, t]) == int(d) + 2 * int(reached), (i, t)
            if d:
                episode += 1
                o = begin()
    # invariants over all 131,072 samples
    bt = tr.buf
    assert torch.isfinite(bt["rew"]).all() and torch.isfinite(bt["val"]).all() and tr.nan_count.item() == 0
    assert torch.equal(bt["keep"][:, 1:], 1 - bt["done"][:, :-1]) and bool((bt["keep"][:, 0] == 1).all())
    assert int(bt["act"].min()) >= 0 and int(bt["act"].max()) <= 4
    # the stash the rollout emitted is the forward pass of the same parameters (what PPO epoch 0 adopts)
    from uavppo import ops
    v = tr.policy.views
    y, _, _, _ = ops.lstm_fwd(bt["obs"][:48].contiguous(), bt["keep"][:48].contiguous(), tr.h0[0][:48].contiguous(),
                              tr.c0[0][:48].contiguous(), v["lstm.weight_ih_l0"], v["lstm.weight_hh_l0"],
                              v["lstm.bias_ih_l0"], v["lstm.bias_hh_l0"])
    assert torch.allclose(tr.work["y0"][:48], y, atol=3e-6)


def test_c4_iteration_is_deterministic(c4):
    from uavppo.trainer import VecPPOTrainer
    tr, bank, src, _ = c4
    outs = []
    for _ in range(2):
        t2 = VecPPOTrainer(tr.N, tr.T, "lstm", hidden=128, variant="v2.1", device=DEV, seed=1234, bank=tr.bank,
                           bank_sources=tr.bank_sources, use_curriculum=False, epochs=2)
        t2.radius = 90.0
        t2.reset()
        t2.train_iteration()
        outs.append((t2.policy.flat.clone(), t2.loss_sums.clone(), t2.buf["obs"].clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert torch.equal(outs[0][2], tr.buf["obs"])           # and the same rollout as the fixture's


def test_c4_whole_iteration_matches_oracle(c4):
    """C4's per-GPU iteration (1024 x 128, h = 128, sigma = 15 bank, radius 90 so that episodes end inside the rollout):
    update on the rollout's own buffers against the oracle update -- losses, gradients, norms, parameters."""
    from _iteration_check import update_vs_oracle
    from uavppo.trainer import VecPPOTrainer
    tr, _, _, _ = c4
    t2 = VecPPOTrainer(tr.N, tr.T, "lstm", hidden=128, variant="v2.1", device=DEV, seed=1234, bank=tr.bank,
                       bank_sources=tr.bank_sources, use_curriculum=False)
    t2.radius = 90.0
    t2.reset()
    t2.collect()
    assert torch.equal(t2.buf["obs"], tr.buf["obs"])         # the rollout the row-replay test pinned to the oracle
    m = update_vs_oracle(t2, "c4")
    assert m["samples"] == 131072 and m["episode_ends"] >= 8


# ------------------------------------------------------------------------------------------------------------ C5
C5 = dict(N=4096, T=256, H=256, L=2, K=2)


def test_c5_tile_whole_iteration_matches_oracle():
    """One tile of C5 -- 64 envs x 256 steps, h = 256 x 2, TREND_K = 2, radius 150 (restarts inside the sequence) -- through the
    SAME kernels as the full shape (stepper rollout whose stash epoch 0 adopts, step_fwd_h3 / cell_bwd_h3 / step_bwd_h3 with
    the pipelined two-layer backward, split-fp16 weight-gradient GEMMs, colsum_xw): rollout replayed by the procedural oracle,
    then the whole update against the oracle's two-layer torch-CPU LSTM (nn.LSTM stack semantics, PPOV2.0/model.py:206-212)."""
    from _iteration_check import update_vs_oracle
    from uavppo import ops
    from uavppo.trainer import VecPPOTrainer
    N, T = 64, C5["T"]
    tr = VecPPOTrainer(N, T, "lstm", hidden=C5["H"], layers=C5["L"], variant="v2.1", device=DEV, seed=1234,
                       use_curriculum=False, trend_k=C5["K"])
    tr.radius = 150.0
    tr.reset()
    ora = pr.ProceduralVecEnv(N, 1234, "v2.1", radius=150.0, trend_k=C5["K"])
    obs = ora.reset()
    tr.collect()
    assert tr._rollout_forward_valid and ops.lstm_bwd_caps(DEV, 6 + C5["K"], 256) != 0      # the fp16-split step path
    b = {k: tr.buf[k].cpu().numpy() for k in ("obs", "act", "rew", "done")}
    for t in range(T):
        assert np.array_equal(b["obs"][:, t], obs), t
        obs, rew, done, _, _, _ = ora.step(b["act"][:, t])
        assert np.allclose(b["rew"][:, t], rew.astype(np.float32), atol=1e-6, rtol=0) and np.array_equal(b["done"][:, t] > 0, done)
    m = update_vs_oracle(tr, "c5_tile")
    assert m["samples"] == 16384 and m["episode_ends"] >= 4


@pytest.fixture(scope="module")
def c5():
    from uavppo.trainer import VecPPOTrainer
    tr = VecPPOTrainer(C5["N"], C5["T"], "lstm", hidden=C5["H"], layers=C5["L"], variant="v2.1", device=DEV, seed=1234,
                       use_curriculum=False, trend_k=C5["K"])
    tr.radius = 150.0
    tr.reset()
    tr.collect()
    tr.compute_advantages()
    tr.rollout_heads = tr.work["heads"].clone()          # what the stepper rollout wrote (pol.heads() reuses the buffer)
    # ... and the stash / y of every layer, which PPO epoch 0 adopts (restored by the last test of the module)
    tr.rollout_forward = {f"{k}{l}": tr.work[f"{k}{l}"].clone() for k in ("stash", "y") for l in range(C5["L"])}
    yield tr
    del tr
    torch.cuda.empty_cache()


def _c5_gradient(tr, arith=None, stack=True, rows=None):
    """PPO gradient of the collected buffers: forward over the stored observations, loss, backward.  rows: an env index
    set; the loss gradient of every other env is zeroed before the backward (the loss itself, its 1/n and the forward stay
    whole-batch), and the head-bias gradient is summed from the remaining rows -- the gradient of those envs' samples alone."""
    from uavppo import ops
    b, pol = tr.buf, tr.policy
    n = tr.N * tr.T
    args = (b["act"].reshape(-1), b["logp"].reshape(-1), tr.adv_n.reshape(-1), tr.ret.reshape(-1), b["val"].reshape(-1),
            1.0 / n, 0.2, 0.01)
    ops.set_lstm_arith(arith or "fp16x3")
    pol.use_stack_bwd = stack
    try:
        heads = pol.heads(b["obs"], b["keep"], tr.h0, tr.c0, tr.work)
        loss = torch.zeros(4, dtype=torch.float64, device=DEV)
        dheads = torch.empty(n, 6, device=DEV)
        dbias = torch.empty(6, device=DEV)
        ops.ppo_loss_heads(heads.view(n, -1), *args, loss, dheads, dbias)
        if rows is not None:
            live = torch.zeros(tr.N, dtype=torch.bool, device=DEV)
            live[torch.as_tensor(np.asarray(rows), dtype=torch.int64, device=DEV)] = True
            dheads.view(tr.N, tr.T, -1)[~live] = 0.0
        g = pol.backward(dheads, tr.work, None if rows is not None else dbias).clone()
    finally:
        ops.set_lstm_arith("fp16x3")
        pol.use_stack_bwd = True
    return g, loss, heads.clone()


def test_c5_rollout_invariants_and_tile_independence(c5):
    """The stepper rollout at 4096 x 256: invariants over the 1 M samples; the first 64 envs (one tile of the step
    kernels) equal, bit for bit, a 64-env job with the same seed (draws are keyed by the GLOBAL env index, tiles are
    independent problems); the rollout's stash IS the update's forward pass (epoch 0 adopts it)."""
    from uavppo.trainer import VecPPOTrainer
    tr = c5
    b = tr.buf
    assert torch.isfinite(b["rew"]).all() and torch.isfinite(b["val"]).all() and tr.nan_count.item() == 0
    assert torch.equal(b["keep"][:, 1:], 1 - b["done"][:, :-1]) and bool((b["keep"][:, 0] == 1).all())
    assert int(b["done"].sum()) > 100
    # trend channels: obs[6] = obs[2](t) - obs[2](t-1) inside an episode
    o = b["obs"]
    same = b["done"][:, :-1] == 0
    assert torch.equal(o[:, 1:, 6][same], (o[:, 1:, 2] - o[:, :-1, 2])[same])
    small = VecPPOTrainer(64, C5["T"], "lstm", hidden=C5["H"], layers=C5["L"], variant="v2.1", device=DEV, seed=1234,
                          use_curriculum=False, trend_k=C5["K"])
    small.radius = 150.0
    small.reset()
    small.collect()
    for k in ("obs", "act", "rew", "val", "logp", "done", "keep"):
        assert torch.equal(small.buf[k], b[k][:64]), k
    for l in range(C5["L"]):
        assert torch.equal(small.work[f"y{l}"], tr.work[f"y{l}"][:64]), l
    # oracle rows: three envs replayed from the procedural oracle (8 observation channels)
    ora = pr.ProceduralVecEnv(3, 1234, "v2.1", radius=150.0, trend_k=2)
    obs = ora.reset()
    bn = {k: b[k][:3].cpu().numpy() for k in ("obs", "act", "rew", "done")}
    for t in range(C5["T"]):
        assert np.array_equal(bn["obs"][:, t], obs), t
        obs, rew, done, _, _, _ = ora.step(bn["act"][:, t])
        assert np.allclose(bn["rew"][:, t], rew.astype(np.float32), atol=1e-6, rtol=0) and np.array_equal(bn["done"][:, t] > 0, done)


def test_c5_gradient_fp16_split_equals_exact_f32_and_pipelined_equals_per_layer(c5):
    """At the full C5 shape: (a) the whole-batch PPO gradient of the default path (fp16-split step kernels, split
    GEMMs, pipelined two-layer backward) equals the exact-f32 path's to f32 summation noise; (b) the pipelined backward
    (uav_lstm_bwd_stack) equals the per-layer calls BIT for bit; (c) recomputing is deterministic; (d) the heads of the
    recomputed forward equal the ones the stepper rollout wrote."""
    tr = c5
    g_stack, loss_a, heads_a = _c5_gradient(tr)
    assert torch.equal(heads_a.view(-1), tr.rollout_heads.view(-1))                           # (d)
    g_again, loss_b, _ = _c5_gradient(tr)
    assert torch.equal(g_stack, g_again) and torch.equal(loss_a, loss_b)                      # (c)
    g_layers, _, _ = _c5_gradient(tr, stack=False)
    assert torch.equal(g_stack, g_layers)                                                     # (b)
    g_f32, loss_f, heads_f = _c5_gradient(tr, arith="f32_mfma")
    assert torch.isfinite(g_f32).all()
    rel = ((g_stack.double() - g_f32.double()).norm() / g_f32.double().norm()).item()
    assert rel < 3e-5, rel                                                                    # (a)
    assert torch.allclose(heads_a, heads_f, atol=2e-5, rtol=1e-4)
    assert torch.allclose(loss_a[1:3], loss_f[1:3], rtol=1e-6)


# ------------------------------------------------------------------------------------------- C5 full shape against f64
# The tests above compare C5's kernels with each other (or meet the oracle at one 64-env tile).  These meet an f64 oracle
# at the full shape -- 64 step-kernel tiles, weight-gradient reductions over K = N T = 1,048,576 rows of per-(env, step)
# power-of-two scales normalised by the batch-wide maximum, per-sample loss gradients of 1/n ~ 1e-6 -- streamed over env
# chunks (tests/_iteration_check.oracle_gradient_chunked).  Bars, per tensor (max |got - want| over max |want|, floored at
# 1e-2 of the largest entry, as update_vs_oracle (a)): the fp16-split default no worse than 2 x the exact-f32 MFMA path's
# error + 2e-7 (tests/test_gpu_lstm_h256.py), both paths <= 1e-3 per tensor and <= 2e-5 relative L2 (update_vs_oracle (a)).
C5_CHUNK = 256
C5_SUBSETS = {"odd_envs_0_255": np.arange(1, 256, 2),     # zero-gradient rows inside every tile of the first four
              "env_4095": np.array([4095])}              # one live env among 4096: it alone sets the batch-wide scale


def _c5_record(key, value):
    """Print a measurement as one JSON line (pytest -s shows it)."""
    import json
    print(f"[c5_full] {key}: {json.dumps(value)}")


@pytest.fixture(scope="module")
def c5_oracle(c5):
    """The f64 oracle of the C5 buffers at the rollout's parameters (= the first optimiser step's): the 16 aligned 256-env
    chunks, whose sum is the full-batch gradient, and the env sets of C5_SUBSETS.  It is fed the trainer's own advantages and
    returns (test_c5_full_gradient_matches_f64_oracle checks them against the oracle's GAE + normalise), so that the gradient
    comparisons measure the forward, loss and backward kernels alone."""
    from _iteration_check import oracle_gradient_chunked
    tr = c5
    args = (tr.policy, tr.buf, tr.h0, tr.c0, tr.adv_n, tr.ret)
    full = oracle_gradient_chunked(*args, chunk=C5_CHUNK)
    sub = oracle_gradient_chunked(*args, envs=list(C5_SUBSETS.values()))
    _c5_record("oracle", {"chunk_envs": C5_CHUNK, "chunks": len(full["chunks"]), "host_seconds_full": round(full["seconds"], 1),
                          "host_seconds_subsets": round(sub["seconds"], 1), "torch_threads": torch.get_num_threads()})
    return full, dict(zip(C5_SUBSETS, sub["chunks"]))


def _c5_errors(tr, g, want):
    from _iteration_check import grad_errors, named_from_flat
    return grad_errors(named_from_flat(tr.policy, g.cpu()), want)


def _c5_check_bars(e16, e32, tag):
    (p16, r16), (p32, r32) = e16, e32
    for k in p16:
        assert p16[k] <= 2.0 * p32[k] + 2e-7, (tag, k, p16[k], p32[k])
        assert p16[k] <= 1e-3 and p32[k] <= 1e-3, (tag, k, p16[k], p32[k])
    assert r16 <= 2e-5 and r32 <= 2e-5, (tag, r16, r32)


def _c5_round(per):
    return {k: float(f"{v:.3g}") for k, v in per.items()}


def test_c5_full_gradient_matches_f64_oracle(c5, c5_oracle):
    """The whole-batch gradient at C5's full shape, at the rollout's parameters, against the f64 oracle: GAE + normalise over
    the 4096 x 256 buffer, the heads of all 1 M samples, the three losses, and every gradient tensor -- the 8 LSTM tensors
    and the actor / critic weight and bias -- under the default fp16-split arithmetic and the exact-f32 MFMA one."""
    import time
    t0 = time.perf_counter()
    tr = c5
    full, _ = c5_oracle
    N, T = tr.N, tr.T
    n = N * T
    b = {k: tr.buf[k].cpu().numpy() for k in ("rew", "val", "done")}
    assert tr.gae_mode == "reference_exact"
    adv_n, ret = po.normalise(po.gae_reference_exact(b["rew"], b["val"], b["done"]), b["val"])
    got_adv, got_ret = tr.adv_n.cpu().numpy().reshape(-1), tr.ret.cpu().numpy().reshape(-1)
    m = {"adv_max_abs_diff": float(np.abs(got_adv - adv_n.numpy()).max()),
         "ret_max_abs_diff": float(np.abs(got_ret - ret.numpy()).max())}
    assert np.allclose(got_adv, adv_n.numpy(), atol=3e-5, rtol=1e-4), m
    assert np.allclose(got_ret, ret.numpy(), atol=3e-5, rtol=1e-4), m
    want_heads = {"logits": full["logits"], "value": full["value"]}
    e, heads_e, losses = {}, {}, {}
    for mode in ("fp16x3", "f32_mfma"):
        g, loss, heads = _c5_gradient(tr, arith=mode)
        assert torch.isfinite(g).all()
        heads = heads.view(N, T, -1).cpu().double()
        got_heads = {"logits": heads[..., :-1], "value": heads[..., -1]}
        heads_e[mode] = {k: float((got_heads[k] - w).abs().max() / w.abs().max()) for k, w in want_heads.items()}
        losses[mode] = (loss.cpu().numpy()[:3] / n).tolist()
        e[mode] = _c5_errors(tr, g, full["grad"])
        m[mode] = {"grad_rel_l2": e[mode][1], "grad_max_rel_per_tensor": _c5_round(e[mode][0]), "heads": heads_e[mode],
                   "losses": losses[mode]}
    m["losses_oracle"] = full["losses"]
    m["seconds_without_oracle"] = round(time.perf_counter() - t0, 1)
    _c5_record("full_batch", m)
    for mode in e:
        # the policy loss is a mean of O(1) terms that cancels to ~1e-5: absolute tolerance (update_vs_oracle (a))
        assert np.allclose(losses[mode], full["losses"], rtol=2e-6, atol=2e-7), (mode, losses[mode], full["losses"])
    for k in want_heads:
        e16, e32 = heads_e["fp16x3"][k], heads_e["f32_mfma"][k]
        assert e16 <= 2.0 * e32 + 2e-7, (k, e16, e32)
        if e32 <= 5e-6:
            assert e16 <= 5e-6, (k, e16, e32)
    _c5_check_bars(e["fp16x3"], e["f32_mfma"], "full batch")


def test_c5_env_subset_gradients_match_f64_oracle(c5, c5_oracle):
    """The gradient of a subset of the envs' samples at the full shape: forward and loss over the whole batch, the loss
    gradient zeroed outside the subset, the backward over all 4096 envs.  15/16 or more of the 1 M (env, step) rows then
    carry exactly zero gate gradients, the regime of the zero-row block-scale fix, at K = 1 M instead of a few thousand.
    Each of the 16 aligned 256-env chunks, the odd envs of envs 0-255 (zero rows inside every tile) and env 4095 alone
    (one env's scale is the batch-wide maximum), under both arithmetics, against that set's f64 oracle gradient."""
    import time
    t0 = time.perf_counter()
    tr = c5
    full, subs = c5_oracle
    sets = [(f"chunk{c}", np.arange(c * C5_CHUNK, (c + 1) * C5_CHUNK), want) for c, want in enumerate(full["chunks"])]
    sets += [(k, C5_SUBSETS[k], subs[k]) for k in C5_SUBSETS]
    assert len(sets) == 18
    e = {}
    for mode in ("f32_mfma", "fp16x3"):
        for name, rows, want in sets:
            g, _, _ = _c5_gradient(tr, arith=mode, rows=rows)
            assert torch.isfinite(g).all(), (name, mode)
            e[name, mode] = _c5_errors(tr, g, want)
    m = {}
    for mode in ("fp16x3", "f32_mfma"):
        chunks = [e[name, mode] for name, _, _ in sets[:-2]]
        worst = {k: max(range(len(chunks)), key=lambda c: chunks[c][0][k]) for k in chunks[0][0]}
        m[f"chunks_{mode}"] = {"worst_grad_rel_l2": max(c[1] for c in chunks),
                               "worst_max_rel_per_tensor": {k: [float(f"{chunks[c][0][k]:.3g}"), f"chunk{c}"] for k, c in worst.items()}}
        for name in C5_SUBSETS:
            m[f"{name}_{mode}"] = {"grad_rel_l2": e[name, mode][1], "grad_max_rel_per_tensor": _c5_round(e[name, mode][0])}
    m["seconds_without_oracle"] = round(time.perf_counter() - t0, 1)
    _c5_record("env_subsets", m)
    for name, _, _ in sets:
        _c5_check_bars(e[name, "fp16x3"], e[name, "f32_mfma"], name)


def test_c5_update_first_gradient_is_the_checked_gradient(c5):
    """LAST in the module: it runs the update, which changes the fixture's parameters.  The first optimiser step of
    tr.update() -- epoch 0 adopting the stash, y and heads the stepper ROLLOUT wrote -- produces, bit for bit, the default
    gradient the tests above checked against the f64 oracle (which recomputes the forward pass)."""
    tr = c5
    # the checked gradient (recomputing is deterministic: test (c) above).  Running the fp16-split forward last also leaves
    # the library's record of the work stash's h_prev slot as the stepper's, which is how the rollout left it
    g16, loss16, heads16 = _c5_gradient(tr)
    assert torch.equal(heads16.view(-1), tr.rollout_heads.view(-1))
    for l in range(C5["L"]):
        assert torch.equal(tr.work[f"y{l}"], tr.rollout_forward[f"y{l}"]), l
    for k, v in tr.rollout_forward.items():              # what epoch 0 adopts is what the rollout wrote
        tr.work[k].copy_(v)
    tr.work["heads"].copy_(tr.rollout_heads)
    assert tr._rollout_forward_valid
    p_before = tr.policy.flat.clone()
    tr.record = tr.record_grads = True
    tr.log.clear()
    tr.grad_log.clear()
    tr.update()
    torch.cuda.synchronize()
    assert not tr._rollout_forward_valid and len(tr.grad_log) == tr.hp["epochs"]
    g0, p0 = tr.grad_log[0]
    assert torch.equal(p0, p_before)
    assert torch.equal(tr.log[0][0][:3], loss16[:3])
    assert torch.equal(g0, g16), float((g0 - g16).abs().max())
