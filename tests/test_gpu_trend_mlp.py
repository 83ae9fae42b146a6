"""MLP policies with the trend observation channels (6 + trend_k inputs, trend_k = 1 / 2) on the fused MLP kernels:
uav_rollout / uav_greedy_episodes / uav_greedy_episodes_stop with policy_kind 2 and uav_mlp_ppo_grad_trend -- against
torch-CPU autograd, the oracle simulation, an f64 greedy oracle, the layered / step-wise paths, and themselves under
chunking.  -m gpu.

Shapes: partial 16-env tiles (N = 1, 5, 17, 21, 37), more than one workgroup, a partial 32-sample update tile, workgroups that
loop over two update tiles (n = 8300 > 256 CUs x 32), episode ends inside every horizon (the trend history restarts there),
T >= 3 so both lags are live, both k.  Tolerances are those of the tests each case restates (test_gpu_trainer.py,
test_gpu_greedy_eval.py, test_gpu_eval_v11.py, test_gpu_trend_fused.py); seeds were fixed after checking margins and coverage
with the CPU oracles alone, and the tests assert those margins again before they trust agreement."""
import os
import sys

import numpy as np
import pytest
import torch

import _eval_v11_check as ck
from oracle import ppo_oracle as po
from oracle import procedural_oracle as pr
from oracle.env_oracle import FieldBank, OracleVecEnv
from test_gpu_greedy_eval import GAP, TOWARDS, _agree, _bank_env
from test_gpu_trainer import _redraw_kink_samples, cpu_params

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "uav-wrf-les-ppo-lstm_amd")
STD_MARGIN, CONC_MARGIN = 1e-2, 1e-6                     # as tests/test_gpu_eval_v11.py
FILL = 0xA5                                              # what a record buffer holds when nothing ran


@pytest.fixture(scope="module")
def ev():
    if PKG not in sys.path:
        sys.path.insert(0, PKG)
    import evaluate_with_lstm as m
    return m


def _trend_mlp(seed, k, bias=TOWARDS, scale=400.0, trend_scale=20.0):
    """A decisive greedy MLP at 6 + k inputs (test_gpu_greedy_eval's recipe: actor rows of gain 0.01 scaled up, a head bias
    that walks +x / +y), the trend columns of feature.0.weight scaled up so that they decide something (the channels are
    differences of obs[2]: small numbers)."""
    from uavppo.policy import MLPActorCritic
    pol = MLPActorCritic(6 + k, 5, device=DEV, seed=seed)
    pol.views["head.weight"][:5].mul_(scale)
    pol.views["head.bias"][:5].copy_(torch.tensor(bias))
    pol.views["feature.0.weight"][:, 6:].mul_(trend_scale)
    return pol


def _p64(pol):
    return {k: v.detach().cpu().double() for k, v in pol.named_views().items()}


def _logits64(p, state):
    with torch.no_grad():
        return po.mlp_forward(p, torch.from_numpy(np.asarray(state, np.float64))[None])[2][0].numpy()


# ---------------------------------------------------------------------------------------------- 1. gradient
@pytest.mark.parametrize("mode", ["fp16x3", "f32_mfma"])
@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("n", [1, 7, 33, 100, 8300])
def test_fused_trend_mlp_gradient_matches_oracle_and_layered_path(n, k, mode):
    """test_gpu_trainer.py::test_fused_mlp_gradient_matches_oracle_and_layered_path at 7 and 8 inputs, in both arithmetics:
    uav_mlp_ppo_grad_trend vs torch-CPU autograd and vs the layer-by-layer HIP path.  The trend columns are signed and small,
    as differences of obs[2] are.  db1 (feature.0.bias: the B operand's valid-sample column) and the new columns of dW1 are
    checked on their own."""
    from uavppo import ops
    from uavppo.policy import MLPActorCritic
    D = 6 + k
    pol = MLPActorCritic(D, 5, device=DEV, seed=n)
    with torch.no_grad():        # non-trivial LayerNorm parameters and biases
        g = torch.Generator().manual_seed(1)
        for key in ("feature.0.bias", "feature.1.bias", "feature.3.bias", "feature.4.bias", "head.bias"):
            pol.views[key].copy_(torch.randn(pol.views[key].shape, generator=g) * 0.2)
        for key in ("feature.1.weight", "feature.4.weight"):
            pol.views[key].copy_(1 + 0.3 * torch.randn(pol.views[key].shape, generator=g))
        pol.views["head.weight"].mul_(20.0)
    rng = np.random.RandomState(n + k)
    obs = rng.rand(n, D).astype(np.float32)
    act = rng.randint(0, 5, n).astype(np.int32)
    adv = rng.randn(n).astype(np.float32)
    ret = rng.randn(n).astype(np.float32)
    vo = rng.randn(n).astype(np.float32)
    lp = (np.log(0.2) + 0.3 * rng.randn(n)).astype(np.float32)
    trend = (0.05 * rng.randn(n, k)).astype(np.float32)
    for _ in range(50):          # the trend columns keep their own distribution where a redraw is needed
        obs[:, 6:] = trend
        before = obs.copy()
        _redraw_kink_samples(pol, rng, obs, act, lp, vo, ret)
        rows = np.flatnonzero((obs != before).any(1))
        if rows.size == 0:
            break
        trend[rows] = (0.05 * rng.randn(rows.size, k)).astype(np.float32)
    else:
        raise AssertionError("could not draw observations away from the loss's kinks")
    d = lambda a: torch.from_numpy(a).to(DEV)
    sums = torch.zeros(4, dtype=torch.float64, device=DEV)
    with ops.lstm_arith(mode):
        ops.mlp_ppo_grad_trend(pol.flat, d(obs), d(act), d(lp), d(adv), d(ret), d(vo), 1.0 / n, 0.2, 0.01, sums, pol.grad, k)
        got = {key: v.detach().cpu().clone() for key, v in pol.named_grads().items()}
        got_flat = pol.grad.clone()
    got_sums = sums.cpu().numpy()
    # oracle
    leaf = {key: v.detach().cpu().clone().requires_grad_(True) for key, v in pol.named_views().items()}
    probs, value, _ = po.mlp_forward(leaf, torch.from_numpy(obs))
    total, pl, vl, ent = po.ppo_losses(probs, value, torch.from_numpy(act), torch.from_numpy(lp), torch.from_numpy(adv),
                                       torch.from_numpy(ret), torch.from_numpy(vo))
    total.backward()
    want_sums = [float(pl.detach()), float(vl.detach()), float(ent.detach())]
    print("losses", got_sums[:3] / n, want_sums)
    assert np.allclose(got_sums[:3] / n, want_sums, rtol=2e-5, atol=1e-6) and got_sums[3] == 0
    bound = lambda scale: (2e-5 + 2e-7 * np.sqrt(n)) * scale + 1e-9
    for key in leaf:
        scale = leaf[key].grad.abs().max().item() + 1e-12
        err = (got[key] - leaf[key].grad).abs().max().item()
        print(key, "err", err, "bound", bound(scale))
        # f32 sums over n samples on both sides, in different orders: rounding grows like sqrt(n) * 2^-24
        assert err <= bound(scale), (key, err, scale)
    # the db1 route and the new columns, on their own
    gb, gw = got["feature.0.bias"], got["feature.0.weight"][:, 6:]
    wb, ww = leaf["feature.0.bias"].grad, leaf["feature.0.weight"].grad[:, 6:]
    assert gw.shape == (256, k) and (gb != 0).any() and (gw != 0).any()
    assert (gb - wb).abs().max().item() <= bound(wb.abs().max().item() + 1e-12)
    assert (gw - ww).abs().max().item() <= bound(ww.abs().max().item() + 1e-12)
    # layer-by-layer HIP path
    heads = pol.heads(d(obs))
    dheads = torch.empty(n, 6, device=DEV)
    s2 = torch.zeros(4, dtype=torch.float64, device=DEV)
    ops.ppo_loss_heads(heads, d(act), d(lp), d(adv), d(ret), d(vo), 1.0 / n, 0.2, 0.01, s2, dheads)
    g2 = pol.backward(dheads).clone()
    print("layered max diff", (got_flat - g2).abs().max().item(), "max|g|", g2.abs().max().item())
    assert torch.allclose(got_flat, g2, rtol=2e-4, atol=2e-6 * g2.abs().max().item())
    assert np.allclose(got_sums, s2.cpu().numpy(), rtol=2e-5)


# ---------------------------------------------------------------------------------------------- 2. the 6-input form
@pytest.mark.parametrize("n", [100, 8300])
def test_trend_gradient_entry_with_k0_is_the_6_input_kernel(n):
    from uavppo import ops
    from uavppo.policy import MLPActorCritic
    pol = MLPActorCritic(6, 5, device=DEV, seed=3)
    pol.views["head.weight"].mul_(20.0)
    rng = np.random.RandomState(n)
    d = lambda a: torch.from_numpy(a).to(DEV)
    obs, act = d(rng.rand(n, 6).astype(np.float32)), d(rng.randint(0, 5, n).astype(np.int32))
    adv, ret, vo = (d(rng.randn(n).astype(np.float32)) for _ in range(3))
    lp = d((np.log(0.2) + 0.3 * rng.randn(n)).astype(np.float32))
    out = []
    for trend in (False, True):
        sums = torch.zeros(4, dtype=torch.float64, device=DEV)
        grad = torch.full_like(pol.flat, float("nan"))
        if trend:
            ops.mlp_ppo_grad_trend(pol.flat, obs, act, lp, adv, ret, vo, 1.0 / n, 0.2, 0.01, sums, grad, 0)
        else:
            ops.mlp_ppo_grad(pol.flat, obs, act, lp, adv, ret, vo, 1.0 / n, 0.2, 0.01, sums, grad)
        out.append((grad, sums))
    assert torch.isfinite(out[0][0]).all() and (out[0][0] != 0).any()
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])


def test_kind2_rollout_with_k0_fills_what_kind0_fills():
    from uavppo import ops
    from uavppo.trainer import VecPPOTrainer
    N, T = 19, 12
    a, b = (VecPPOTrainer(N, T, "mlp", device=DEV, seed=6, use_curriculum=False, gae_mode="standard", log_info=True)
            for _ in range(2))
    for tr, trend in ((a, False), (b, True)):
        tr.radius = 300.0
        tr.reset()
        ops.rollout_mlp(tr.env_state, N, tr.env_cfg(), tr.policy.flat, T, 0, tr.cur_obs, tr.buf, last_val=tr.last_val,
                        nan_count=tr.nan_count, info=tr.info, trend=trend)
    for key in a.buf:
        assert torch.equal(a.buf[key], b.buf[key]), key
    assert torch.equal(a.cur_obs, b.cur_obs) and torch.equal(a.last_val, b.last_val) and torch.equal(a.info, b.info)
    assert torch.equal(a.env_state, b.env_state)
    assert a.buf["done"].sum() >= 1 and (a.buf["rew"] != 0).any()


# ---------------------------------------------------------------------------------------------- 3. rollout vs the oracle
@pytest.mark.parametrize("N,T,k", [(5, 40, 1), (37, 70, 2)])
def test_fused_trend_mlp_rollout_matches_oracle_simulation(N, T, k):
    """test_gpu_trainer.py::test_fused_mlp_rollout_matches_oracle_simulation with trend_k = k: uav_rollout policy_kind 2 vs a
    step-by-step oracle simulation on injected noise + forced actions + a materialised bank: env bit-exact (all 6 + k
    observation columns), policy outputs to f32 tolerance; and the step-wise HIP path fills identical buffers."""
    from uavppo.trainer import VecPPOTrainer
    bank = FieldBank.from_seed(3 * N, "v2.0", seed=31)
    mk = lambda: VecPPOTrainer(N, T, "mlp", variant="v2.0", device=DEV, seed=5, bank=bank.interleaved(),
                               bank_sources=bank.sources, gae_mode="standard", use_curriculum=False, log_info=True, trend_k=k)
    tr, ts = mk(), mk()
    assert tr.fused_mlp and tr.rollout_route() == "fused_mlp"
    ts.fused_mlp = False
    for t_ in (tr, ts):
        t_.radius = 45.0
        t_.reset()
    rng = np.random.RandomState(2)
    noise = rng.randn(N, T, 2)
    ora = OracleVecEnv(N, bank, "v2.0", radius=45.0, trend_k=k)
    obs = ora.reset()
    assert obs.shape == (N, 6 + k) and np.array_equal(tr.cur_obs.cpu().numpy(), obs)
    p = cpu_params(tr.policy)
    assert p["feature.0.weight"].shape == (256, 6 + k)
    acts = np.zeros((N, T), np.int32)
    want = {key: [] for key in ("obs", "rew", "done", "val", "logp")}
    for t in range(T):
        a = []
        for i, e in enumerate(ora.envs):              # home in on the source for a while (forces episode ends), then random
            dd = e.source - e.pos
            hom = (3 if dd[0] > 0 else 4) if abs(dd[0]) > abs(dd[1]) else (1 if dd[1] > 0 else 2)
            a.append(hom if (t < 30 or i % 2 == 0) else int(rng.randint(0, 5)))
        acts[:, t] = a
        with torch.no_grad():
            probs, value, _ = po.mlp_forward(p, torch.from_numpy(obs))
            lp = po.categorical_logp(probs, torch.tensor(a))
        want["obs"].append(obs.copy())
        want["val"].append(value[:, 0].numpy().copy())
        want["logp"].append(lp.numpy().copy())
        obs, rew, done, reached, info, term = ora.step(np.array(a), noise[:, t])
        want["rew"].append(rew.astype(np.float32))
        want["done"].append(done.astype(np.float32))
    with torch.no_grad():
        _, v_last, _ = po.mlp_forward(p, torch.from_numpy(obs))
    fa, nz = torch.from_numpy(acts).to(DEV), torch.from_numpy(noise).to(DEV)
    tr.collect(forced_act=fa, noise=nz)
    ts.collect(forced_act=fa, noise=nz)
    b = {key: v.cpu().numpy() for key, v in tr.buf.items()}
    w_obs = np.stack(want["obs"], 1)
    assert b["obs"].shape == (N, T, 6 + k) and np.array_equal(b["obs"], w_obs)
    assert (b["obs"][..., 6:] != 0).any(), "the trend channels never moved"
    assert np.array_equal(b["done"], np.stack(want["done"], 1))
    assert np.array_equal(b["act"], acts)
    assert np.allclose(b["rew"], np.stack(want["rew"], 1), atol=1e-6, rtol=0)
    assert np.allclose(b["val"], np.stack(want["val"], 1), atol=2e-5, rtol=1e-4)
    assert np.allclose(b["logp"], np.stack(want["logp"], 1), atol=2e-5, rtol=1e-4)
    assert np.array_equal(tr.cur_obs.cpu().numpy(), obs)
    assert np.allclose(tr.last_val.cpu().numpy(), v_last[:, 0].numpy(), atol=2e-5, rtol=1e-4)
    assert b["done"].sum() >= 2 and tr.nan_count.item() == 0
    for key in ("obs", "act", "done", "flags"):
        assert torch.equal(tr.buf[key], ts.buf[key]), key
    assert torch.equal(tr.cur_obs, ts.cur_obs)
    for key in ("rew", "val", "logp"):
        assert torch.allclose(tr.buf[key], ts.buf[key], atol=2e-5, rtol=1e-4), key
    assert torch.allclose(tr.info, ts.info, atol=1e-4) and torch.allclose(tr.last_val, ts.last_val, atol=2e-5)


# ---------------------------------------------------------------------------------------------- 4. rollout logp = update's forward
def test_trend_rollout_logp_is_the_updates_first_forward():
    """The exact half of test_gpu_trainer.py::test_fused_mlp_rollout_logp_is_the_updates_first_forward at trend_k = 2: rollout
    and update run the same forward code in the same order, so at epoch 0 the ratio is exactly 1 and the policy loss is
    exactly -mean(adv_n)."""
    from uavppo.trainer import VecPPOTrainer
    N, T = 48, 16
    tr = VecPPOTrainer(N, T, "mlp", device=DEV, seed=9, use_curriculum=False, epochs=1, trend_k=2)
    assert tr.fused_mlp
    tr.collect()
    assert (tr.buf["obs"][..., 6:] != 0).any()
    tr.record = True
    tr.update()
    s = tr.log[0][0].cpu().numpy()
    assert abs(s[0] / (N * T) + tr.adv_n.double().mean().item()) < 1e-9


# ---------------------------------------------------------------------------------------------- 5. edge shapes
@pytest.mark.parametrize("N,T,k", [(1, 3, 1), (17, 1, 2)])
def test_fused_trend_mlp_edge_shapes(N, T, k):
    from uavppo.trainer import VecPPOTrainer
    tr = VecPPOTrainer(N, T, "mlp", device=DEV, seed=N + T, epochs=2, trend_k=k)
    assert tr.fused_mlp
    p0 = tr.policy.flat.clone()
    for _ in range(2):
        tr.train_iteration()
    pl, vl, ent = tr.losses()
    assert np.isfinite([pl, vl, ent]).all() and torch.isfinite(tr.policy.flat).all()
    assert (tr.policy.flat - p0).abs().max() > 0
    b = {key: v.cpu().numpy() for key, v in tr.buf.items()}
    assert b["obs"].shape == (N, T, 6 + k)
    assert np.allclose(tr.adv.cpu().numpy(), po.gae_reference_exact(b["rew"], b["val"], b["done"]), rtol=2e-5, atol=2e-5)


# ---------------------------------------------------------------------------------------------- 6. greedy vs the f64 oracle
def _oracle_mlp(pol, bank, N, cap, noise, k):
    """test_gpu_greedy_eval._oracle_lstm without the state: one f64 episode per env, argmax of the logits.
    Returns steps, stopped, deviations, reached, smallest top-2 logit gap."""
    p = _p64(pol)
    ora = OracleVecEnv(N, bank, "v2.0", radius=50.0, trend_k=k)
    ora.reset()
    steps, devs, reached, gap = [], [], [], np.inf
    for i, e in enumerate(ora.envs):
        state, t, done, rc = e.obs(), 0, False, False
        while not done and t < cap:
            z = _logits64(p, state)
            top = np.sort(z)[-2:]
            gap = min(gap, float(top[1] - top[0]))
            state, _, done, rc, _ = e.step(int(np.argmax(z)), noise[t, i])
            t += 1
        steps.append(t)
        reached.append(rc)
        devs.append(float(np.linalg.norm(np.asarray(e.pos, np.float64) - np.asarray(e.source, np.float64))))
    return np.asarray(steps), np.zeros(N, bool), np.asarray(devs), np.asarray(reached), gap


@pytest.mark.parametrize("k,bank_seed,pol_seed", [(1, 94, 2), (2, 94, 1)])
def test_fused_greedy_trend_mlp_matches_f64_oracle(ev, k, bank_seed, pol_seed):
    """evaluate(fused=True) of a 6 + k input MLP against f64 oracle episodes.  Margins of the two cases, found with the oracle
    alone: k = 1 smallest top-2 gap 4.8e-3, 2 envs reach the source, 19 run to the cap, zeroing the trend column changes 2
    envs' step counts; k = 2 gap 1.4e-3, 3 reach, 18 at the cap, 3 change."""
    N, CAP = 21, 120
    noise = np.random.RandomState(256 + k).randn(CAP, N, 2)
    bank, env = _bank_env(N, "v2.0", bank_seed, 3, trend_k=k)
    pol = _trend_mlp(pol_seed, k)
    steps, stopped, devs, reached, gap = _oracle_mlp(pol, bank, N, CAP, noise, k)
    assert gap > GAP, f"oracle's smallest top-2 logit gap {gap:g}: agreement would be luck"
    assert reached.any() and (steps == CAP).any(), (reached.sum(), steps)       # some reach the source, some time out
    blind = _trend_mlp(pol_seed, k)
    blind.views["feature.0.weight"][:, 6:].zero_()
    steps_blind = _oracle_mlp(blind, bank, N, CAP, noise, k)[0]
    assert (steps_blind != steps).any(), "the trend channels decide nothing here"
    assert ev.fused_refusal(pol, env) is None
    got = ev.evaluate(pol, env, noise=torch.from_numpy(noise).to(DEV), max_steps=CAP, fused=True)
    _agree(got, steps, stopped, devs)
    assert np.array_equal(got["success"], devs <= ev.SUCCESS_DISTANCE_THRESHOLD)


# ---------------------------------------------------------------------------------------------- 7. chunking
@pytest.mark.parametrize("stop", [False, True])
@pytest.mark.parametrize("k", [1, 2])
def test_chunking_is_invisible_for_a_trend_mlp(k, stop):
    """Three calls of 40 steps give what one call of 120 gives, bit for bit: records, blob, cur_obs (6 + k wide), active,
    nan_count and, with the stop rule, the window buffers."""
    from uavppo import ops
    N, CAP = 21, 120
    pol = _trend_mlp(2, k)
    noise = torch.from_numpy(np.random.RandomState(5).randn(N, CAP, 2)).to(DEV)
    rule = ops.make_stop_rule()
    runs = []
    for chunk in (CAP, 40):
        _, env = _bank_env(N, "v2.0", 13, 3, trend_k=k)
        env.current_radius = 200.0                        # episodes end inside the cap
        env.reset()
        cur = env.obs.clone()
        assert cur.shape == (N, 6 + k)
        active = torch.ones(N, dtype=torch.uint8, device=DEV)
        win = torch.zeros(N, rule.window, 2, device=DEV)
        cnt = torch.zeros(N, dtype=torch.int32, device=DEV)
        nan = torch.zeros(1, dtype=torch.int32, device=DEV)
        recs = {"act": [], "obs": [], "pos": [], "flags": []}
        for t0 in range(0, CAP, chunk):
            r = ops.greedy_recs(N, chunk, 6 + k, DEV)
            nz = noise[:, t0:t0 + chunk].contiguous()
            if stop:
                ops.greedy_episodes_stop(env.state, N, env.cfg(), pol.flat, 0, chunk, cur, None, None, active, r, rule, win, cnt,
                                         noise=nz, nan_count=nan, trend=True)
            else:
                ops.greedy_episodes(env.state, N, env.cfg(), pol.flat, 0, chunk, cur, None, None, active, r, noise=nz,
                                    nan_count=nan, trend=True)
            for key in recs:
                recs[key].append(r[key])
        recs = {key: torch.cat(v, 1).cpu() for key, v in recs.items()}
        runs.append((recs, [env.state.cpu(), cur.cpu(), active.cpu(), win.cpu(), cnt.cpu(), int(nan.item())]))
    (ra, fa), (rb, fb) = runs
    for key in ra:
        assert torch.equal(ra[key], rb[key]), key
    for i, (x, y) in enumerate(zip(fa, fb)):
        assert torch.equal(x, y) if torch.is_tensor(x) else x == y, i
    flags = ra["flags"]
    assert fa[5] == 0
    ended = (flags & (9 if stop else 1)) != 0
    assert ended[:, :80].any(), "no episode ended before the last chunk: freezing across chunks went untested"
    frozen = (flags & 4) != 0
    assert frozen.any() and (flags[frozen] == 4).all()
    assert (ra["obs"][..., 6:][~frozen] != 0).any()
    assert (ra["obs"][frozen] == 0).all() and (ra["pos"][frozen] == 0).all() and (ra["act"][frozen] == -1).all()


# ---------------------------------------------------------------------------------------------- 8. ModelEvaluator
def _oracle_v11_trend_mlp(pol, N, cap, seed, k):
    """test_gpu_trend_fused._oracle_v11_trend for an MLP: (steps, stopped, success, smallest top-2 gap, std margin,
    concentration margin) of f64 greedy episodes on a procedural v1.1 env with the stop rule and the env's own step noise."""
    p = _p64(pol)
    ora = pr.ProceduralVecEnv(N, seed, "v1.1", trend_k=k)
    ora.reset()
    steps, stopped, success = [], [], []
    gap, std_margin, conc_margin = np.inf, np.inf, np.inf
    for i, e in enumerate(ora.envs):
        state, traj, t, over, fired = e.obs(), [], 0, False, False
        while not over and t < cap:
            z = _logits64(p, state)
            top = np.sort(z)[-2:]
            gap = min(gap, float(top[1] - top[0]))
            state, _, over, _, _ = e.step(int(np.argmax(z)), pr.step_normals(seed, i, 0, e.steps))
            traj.append(np.asarray(e.pos, np.float32))
            fired, v = ck.rule(traj, state[2])
            if len(traj) >= ck.WINDOW:
                std_margin = min(std_margin, abs(float(v) - ck.POS_STD_MAX))
                conc_margin = min(conc_margin, abs(float(ck.conc_high(state[2])[1]) - ck.CONC_MIN) /
                                  (ck.CONC_PEAK * ck.CONC_PEAK * ck.CONC_COEF))
            over = over or fired
            t += 1
        d = traj[-1].astype(np.float64) - np.asarray(e.source, np.float64)
        steps.append(t)
        stopped.append(fired)
        success.append(float(np.sqrt(d[0] * d[0] + d[1] * d[1])) < 50.0)
    return np.asarray(steps), np.asarray(stopped), np.asarray(success), gap, std_margin, conc_margin


def test_model_evaluator_runs_a_trend_mlp_fused():
    """ModelEvaluator on a trend_k = 1 env with a 7-input MLP: the fused run (uav_greedy_episodes_stop, policy_kind 2) and the
    step-wise run give the same steps / stops / success -- those of the f64 oracle (its margins here: gap 1.4e-3, std 1.4e-2,
    concentration 4.8e-5; the rule stops 14 of 21 envs)."""
    if PKG not in sys.path:
        sys.path.insert(0, PKG)
    import evaluate_model as em
    from evaluate_with_lstm import fused_refusal
    from uavppo.vec_env import VecMethaneEnv
    N, CAP, k = 21, 300, 1
    pol = _trend_mlp(3, k)
    env = VecMethaneEnv(N, "v1.1", DEV, trend_k=k)
    steps, stopped, success, gap, std_margin, conc_margin = _oracle_v11_trend_mlp(pol, N, CAP, env.seed, k)
    assert gap > GAP and std_margin >= STD_MARGIN and conc_margin > CONC_MARGIN, (gap, std_margin, conc_margin)
    assert stopped.any() and (~stopped).any() and success.any() and np.ptp(steps) > 0          # the rule settles some, not all
    evl = em.ModelEvaluator(pol, N, DEV, env=env)
    assert fused_refusal(pol, env) is None
    fused = evl.run_evaluation(max_steps=CAP, fused=True, csv_path=None)
    step = evl.run_evaluation(max_steps=CAP, fused=False, csv_path=None)
    for key in ("steps", "stopped_early", "success"):
        assert np.array_equal(fused[key], step[key]), key
    assert np.array_equal(fused["steps"], steps) and np.array_equal(fused["stopped_early"], stopped)
    assert np.array_equal(fused["success"], success)
    assert np.allclose(fused["deviations"], step["deviations"], rtol=0, atol=2e-3)


# ---------------------------------------------------------------------------------------------- 9. generate_expert_data
def test_generate_expert_data_of_a_trend_mlp(monkeypatch):
    """A 7-input MLP: states of width 7 from the fused kernel, equal to the pairs the step-wise loop cuts for the same policy
    and environment."""
    if PKG not in sys.path:
        sys.path.insert(0, PKG)
    import generate_expert_data as ged
    from uavppo.vec_env import VecMethaneEnv
    N, steps, seed = 12, 120, 5
    pol = _trend_mlp(5, 1)
    assert ged.fused_refusal(pol, VecMethaneEnv(N, "v2.0", DEV, seed=seed, trend_k=1)) is None
    states, actions = ged.generate_expert_data(pol, num_episodes=N, variant="v2.0", seed=seed, max_steps=steps, out=None)
    assert states.shape[1] == 7 and states.dtype == np.float32 and actions.dtype == np.int64
    assert 0 < len(actions) <= N * steps and actions.min() >= 0 and actions.max() < 5
    assert (states[:, 6] != 0).any()
    monkeypatch.setattr(ged, "fused_refusal", lambda policy, env: "step-wise wanted")
    s2, a2 = ged.generate_expert_data(pol, num_episodes=N, variant="v2.0", seed=seed, max_steps=steps, out=None)
    assert np.array_equal(states, s2) and np.array_equal(actions, a2)


# ---------------------------------------------------------------------------------------------- 10. refusals
def test_trend_mlp_refusals_run_nothing(ev):
    from uavppo import ops
    from uavppo.policy import MLPActorCritic
    from uavppo.vec_env import VecMethaneEnv
    N, T = 16, 4
    env2, env1, env0 = (VecMethaneEnv(N, "v2.0", DEV, trend_k=k) for k in (2, 1, 0))
    mlp6, mlp7 = MLPActorCritic(6, 5, device=DEV, seed=1), MLPActorCritic(7, 5, device=DEV, seed=1)
    n6, n7 = ops.mlp_param_count(6), ops.mlp_param_count(7)
    env1.reset()
    obs_before = env1.obs.clone()
    recs = {"act": torch.full((N, T), FILL, dtype=torch.int32, device=DEV), "obs": torch.full((N, T, 7), float(FILL), device=DEV),
            "pos": torch.full((N, T, 2), float(FILL), device=DEV), "flags": torch.full((N, T), FILL, dtype=torch.uint8, device=DEV)}
    act = torch.ones(N, dtype=torch.uint8, device=DEV)
    cnt = torch.zeros(N, dtype=torch.int32, device=DEV)
    win = torch.zeros(N, 10, 2, device=DEV)
    # kind 2 on a handle that is not in fp16x3
    with ops.lstm_arith("f32_mfma"):
        with pytest.raises(RuntimeError, match="uav_greedy_episodes: the fused greedy kernels exist in the fp16x3 arithmetic only"):
            ops.greedy_episodes(env1.state, N, env1.cfg(), mlp7.flat, 0, T, env1.obs, None, None, act, recs, trend=True)
        with pytest.raises(RuntimeError, match="uav_greedy_episodes_stop: the fused greedy kernels exist in the fp16x3"):
            ops.greedy_episodes_stop(env1.state, N, env1.cfg(), mlp7.flat, 0, T, env1.obs, None, None, act, recs,
                                     ops.make_stop_rule(), win, cnt, trend=True)
    # a 6-input parameter vector offered as kind 2 on a trend_k = 1 env: the wrapper's length check names both numbers
    with pytest.raises(RuntimeError, match=f"{n6} floats.*7 inputs.*trend_k = 1.*{n7}"):
        ops.greedy_episodes(env1.state, N, env1.cfg(), mlp6.flat, 0, T, env1.obs, None, None, act, recs, trend=True)
    bufs = {"obs": torch.full((N, T, 7), float(FILL), device=DEV), "act": torch.full((N, T), FILL, dtype=torch.int32, device=DEV),
            "flags": torch.full((N, T), FILL, dtype=torch.uint8, device=DEV)}
    for key in ("rew", "val", "logp", "done"):
        bufs[key] = torch.full((N, T), float(FILL), device=DEV)
    nan = torch.zeros(1, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match=f"{n6} floats.*7 inputs.*trend_k = 1.*{n7}"):
        ops.rollout_mlp(env1.state, N, env1.cfg(), mlp6.flat, T, 0, env1.obs, bufs, nan_count=nan, trend=True)
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=DEV)
    sums, grad = torch.full((4,), float(FILL), dtype=torch.float64, device=DEV), torch.full_like(mlp7.flat, float(FILL))
    with pytest.raises(RuntimeError, match=f"{n6} floats.*7 inputs.*trend_k = 1.*{n7}"):
        ops.mlp_ppo_grad_trend(mlp6.flat, z(T, 7), z(T, dt=torch.int32), z(T), z(T), z(T), z(T), 1.0 / T, 0.2, 0.01, sums, grad, 1)
    # trend_k = 3: the wrapper, and the ABI underneath it
    with pytest.raises(RuntimeError, match="trend_k=3"):
        ops.mlp_ppo_grad_trend(mlp7.flat, z(T, 9), z(T, dt=torch.int32), z(T), z(T), z(T), z(T), 1.0 / T, 0.2, 0.01, sums, grad, 3)
    from uavppo import _lib
    p = lambda t: _lib.C.c_void_p(t.data_ptr())
    h = ops.Context.get(DEV).handle
    rc = _lib.lib().uav_mlp_ppo_grad_trend(h, p(mlp7.flat), p(z(T, 9)), p(z(T, dt=torch.int32)), p(z(T)), p(z(T)), p(z(T)),
                                           p(z(T)), T, 3, 1.0 / T, 0.2, 0.01, p(sums), p(grad), None)
    assert rc != 0 and b"uav_mlp_ppo_grad_trend: trend_k=3" in _lib.lib().uav_last_error()
    cfg3 = env1.cfg()
    cfg3.trend_k = 3
    with pytest.raises(RuntimeError, match="trend_k must be 0, 1 or 2"):
        _raw_greedy_kind2(env1, cfg3, mlp7, N, T, recs, act)
    torch.cuda.synchronize()
    assert (recs["flags"] == FILL).all() and (recs["act"] == FILL).all() and (recs["obs"] == FILL).all()
    assert (bufs["flags"] == FILL).all() and (bufs["obs"] == FILL).all() and (bufs["rew"] == FILL).all()
    assert (sums == FILL).all() and (grad == FILL).all() and int(cnt.sum()) == 0 and int(nan.item()) == 0
    assert torch.equal(env1.obs, obs_before) and (act == 1).all()
    # fused_refusal: both widths and trend_k
    why = ev.fused_refusal(mlp7, env2)
    assert why is not None and "7 inputs" in why and "8 features" in why and "trend_k = 2" in why
    with pytest.raises(RuntimeError, match="7 inputs.*8 features.*trend_k = 2"):
        ev.evaluate(mlp7, env2, max_steps=5, fused=True)
    why = ev.fused_refusal(mlp7, env0)
    assert why is not None and "7 inputs" in why and "6 features" in why and "trend_k = 0" in why
    assert ev.fused_refusal(mlp7, env1) is None and ev.fused_refusal(mlp6, env0) is None
    assert ev.fused_refusal(MLPActorCritic(8, 5, device=DEV, seed=1), env2) is None


def _raw_greedy_kind2(env, cfg, pol, N, T, recs, act):
    """uav_greedy_episodes with policy_kind 2 and a cfg the wrapper's own checks would not let through (trend_k = 3)."""
    from uavppo import _lib, ops
    p = lambda t: _lib.C.c_void_p(t.data_ptr())
    nan = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.check(_lib.lib().uav_greedy_episodes(ops.Context.get(DEV).handle, p(env.state), N, _lib.C.byref(cfg), 2, p(pol.flat), 0, T,
                                             p(env.obs), None, None, p(act), None, p(recs["act"]), p(recs["obs"]), p(recs["pos"]),
                                             p(recs["flags"]), p(nan), None), "uav_greedy_episodes")
