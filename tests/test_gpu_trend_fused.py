"""Single-layer h = 64 / 128 LSTM policies with the trend observation channels (obs_dim = 6 + trend_k, trend_k = 1 / 2) on the
fused kernels: uav_rollout (training rollout, with the stash that PPO epoch 0 adopts, h_prev slot included) and
uav_greedy_episodes / uav_greedy_episodes_stop (evaluate(), ModelEvaluator, generate_expert_data) -- against the oracle
simulation, the f64 greedy oracle, the step-wise paths, and themselves under chunking.  -m gpu.

Shapes: partial 16-env tiles (N = 5, 19, 21), more than one workgroup, episode ends inside every horizon (the trend history
restarts there), T >= 3 so both lags are live, both k, both H.  Tolerances are those of the tests each case restates
(test_gpu_trainer.py, test_gpu_greedy_eval.py, test_gpu_eval_v11.py); seeds were fixed after checking margins and coverage
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
from test_gpu_greedy_eval import GAP, TOWARDS, _agree, _bank_env, _lstm_policy, _oracle_lstm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "uav-wrf-les-ppo-lstm_amd")
STD_MARGIN, CONC_MARGIN = 1e-2, 1e-6                     # as tests/test_gpu_eval_v11.py


@pytest.fixture(scope="module")
def ev():
    if PKG not in sys.path:
        sys.path.insert(0, PKG)
    import evaluate_with_lstm as m
    return m


def _trend_policy(H, seed, k, bias=TOWARDS):
    """test_gpu_greedy_eval's decisive policy at obs_dim = 6 + k, the trend columns of w_ih scaled up so that they decide
    something (the channels are differences of obs[2]: small numbers)."""
    pol = _lstm_policy(H, seed, obs_dim=6 + k, bias=bias)
    pol.views["lstm.weight_ih_l0"][:, 6:].mul_(20.0)
    return pol


def cpu_params(policy):
    return {k: v.detach().cpu().clone() for k, v in policy.named_views().items()}


# ---------------------------------------------------------------------------------------------- 1. rollout vs the oracle
@pytest.mark.parametrize("H,N,T,k", [(64, 5, 40, 1), (128, 19, 70, 2)])
def test_fused_trend_rollout_matches_oracle_simulation(H, N, T, k):
    """test_gpu_trainer.py::test_fused_rollout_matches_oracle_simulation with trend_k = k: injected noise, forced actions,
    materialised bank; every stored quantity, all 6 + k observation columns included, equals the step-by-step oracle."""
    from uavppo.trainer import VecPPOTrainer
    bank = FieldBank.from_seed(3 * N, "v2.0", seed=31)
    tr = VecPPOTrainer(N, T, "lstm", hidden=H, variant="v2.0", device=DEV, seed=5, bank=bank.interleaved(),
                       bank_sources=bank.sources, gae_mode="standard", use_curriculum=False, trend_k=k)
    tr.radius = 45.0
    tr.reset()
    rng = np.random.RandomState(2)
    noise = rng.randn(N, T, 2)
    ora = OracleVecEnv(N, bank, "v2.0", radius=45.0, trend_k=k)
    obs = ora.reset()
    assert obs.shape == (N, 6 + k) and np.array_equal(tr.cur_obs.cpu().numpy(), obs)
    p = cpu_params(tr.policy)
    assert p["lstm.weight_ih_l0"].shape == (4 * H, 6 + k)
    h = torch.zeros(1, N, H)
    c = torch.zeros(1, N, H)
    acts = np.zeros((N, T), np.int32)
    want = {key: [] for key in ("obs", "rew", "done", "val", "logp", "keep")}
    keep = np.ones(N, np.float32)
    for t in range(T):
        a = []
        for i, e in enumerate(ora.envs):              # home in on the source for a while (forces episode ends), then random
            d = e.source - e.pos
            hom = (3 if d[0] > 0 else 4) if abs(d[0]) > abs(d[1]) else (1 if d[1] > 0 else 2)
            a.append(hom if (t < 30 or i % 2 == 0) else int(rng.randint(0, 5)))
        acts[:, t] = a
        with torch.no_grad():
            km = torch.from_numpy(keep)[None]
            probs, value, _, (h, c) = po.lstm_policy_forward(p, torch.from_numpy(obs)[None], h, c, keep=km)
            lp = po.categorical_logp(probs[0], torch.tensor(a))
        want["obs"].append(obs.copy())
        want["val"].append(value[0].numpy().copy())
        want["logp"].append(lp.numpy().copy())
        want["keep"].append(keep.copy())
        obs, rew, done, reached, info, term = ora.step(np.array(a), noise[:, t])
        want["rew"].append(rew.astype(np.float32))
        want["done"].append(done.astype(np.float32))
        keep = 1.0 - done.astype(np.float32)
    with torch.no_grad():
        km = torch.from_numpy(keep)[None]
        _, v_last, _, (h_end, c_end) = po.lstm_policy_forward(p, torch.from_numpy(obs)[None], h, c, keep=km)
    tr.collect(forced_act=torch.from_numpy(acts).to(DEV), noise=torch.from_numpy(noise).to(DEV))
    assert tr._rollout_forward_valid, "collect() did not take the fused rollout kernel"
    b = {key: v.cpu().numpy() for key, v in tr.buf.items()}
    w_obs = np.stack(want["obs"], 1)
    assert b["obs"].shape == (N, T, 6 + k) and np.array_equal(b["obs"], w_obs)
    assert (w_obs[:, :, 6:] != 0).any(), "the trend channels never moved"
    assert np.array_equal(b["done"], np.stack(want["done"], 1))
    assert np.array_equal(b["keep"], np.stack(want["keep"], 1))
    assert np.array_equal(b["act"], acts)
    assert np.allclose(b["rew"], np.stack(want["rew"], 1), atol=1e-6, rtol=0)
    assert np.allclose(b["val"], np.stack(want["val"], 1), atol=2e-5, rtol=1e-4)
    assert np.allclose(b["logp"], np.stack(want["logp"], 1), atol=2e-5, rtol=1e-4)
    assert np.array_equal(tr.cur_obs.cpu().numpy(), obs)
    assert np.allclose(tr.last_val.cpu().numpy(), v_last[0].numpy(), atol=2e-5, rtol=1e-4)
    km = torch.from_numpy(keep)[:, None]
    assert np.allclose(tr.h[0].cpu().numpy(), (h[0] * km).numpy(), atol=2e-5)
    assert np.allclose(tr.c[0].cpu().numpy(), (c[0] * km).numpy(), atol=2e-5)
    assert b["done"].sum() >= 2 and tr.nan_count.item() == 0


# ---------------------------------------------------------------------------------------------- 2. fused vs step-wise
@pytest.mark.parametrize("H,k", [(64, 1), (128, 2)])
def test_fused_trend_rollout_matches_stepwise(H, k):
    """test_gpu_trainer.py::test_stepwise_lstm_rollout_matches_fused_kernel on a trend env: two schedules of the same
    computation.  The forced actions fan out from the corner in +x / +y, so some envs reach their source (radius 60) and
    restart inside the horizon."""
    from uavppo.trainer import VecPPOTrainer
    N, T = 21, 30
    bank = FieldBank.from_seed(2 * N, "v2.0", seed=41)
    mk = lambda: VecPPOTrainer(N, T, "lstm", hidden=H, device=DEV, seed=8, bank=bank.interleaved(),
                               bank_sources=bank.sources, gae_mode="standard", use_curriculum=False, trend_k=k)
    a, b = mk(), mk()
    a.radius = b.radius = 60.0
    a.reset(); b.reset()
    rng = np.random.RandomState(1)
    fan = rng.rand(N, T) < (np.arange(N)[:, None] + 1.0) / (N + 1)
    fa = torch.from_numpy(np.where(fan, 3, 1).astype(np.int32)).to(DEV)
    nz = torch.from_numpy(rng.randn(N, T, 2)).to(DEV)
    a.collect(forced_act=fa, noise=nz)
    assert a._rollout_forward_valid
    b.h0.copy_(b.h); b.c0.copy_(b.c)
    b._collect_stepwise_lstm(fa, nz)
    assert a.buf["obs"].shape == (N, T, 6 + k)
    for key in ("obs", "act", "done", "keep", "flags"):
        assert torch.equal(a.buf[key], b.buf[key]), key
    assert torch.equal(a.cur_obs, b.cur_obs)
    for key in ("rew", "val", "logp"):
        assert torch.allclose(a.buf[key], b.buf[key], atol=2e-5, rtol=1e-4), key
    assert torch.allclose(a.h, b.h, atol=2e-5) and torch.allclose(a.c, b.c, atol=2e-5)
    assert torch.allclose(a.last_val, b.last_val, atol=2e-5)
    done = a.buf["done"] > 0
    assert int(done[:, :T - 3].sum()) >= 2, "no episode ended inside the horizon"
    assert a.nan_count.item() == 0


# ---------------------------------------------------------------------------------------------- 3. adopted forward pass
def test_epoch0_adopts_the_trend_rollouts_forward_pass():
    """test_gpu_trainer.py::test_epoch0_reuses_rollout_forward with trend_k = 2: the kernel's y and its whole stash, the
    h_prev slot [5H:6H] that uav_lstm_wgrad reads at I = 8 included, equal what uav_lstm_fwd recomputes; an update that adopts
    them lands where one that recomputes the forward pass lands.  Radius 300 makes the envs whose source lies near the
    starting corner end an episode at every step, so keep holds zeros and ones."""
    from uavppo import ops
    from uavppo.trainer import VecPPOTrainer
    H = 128

    def mk(k):
        tr = VecPPOTrainer(40, 24, "lstm", hidden=H, device=DEV, seed=4, use_curriculum=False, epochs=2, trend_k=k)
        tr.radius = 300.0
        tr.reset()
        return tr

    a, b = mk(2), mk(2)
    b.reuse_rollout_forward = False
    a.work["stash0"].fill_(-7.0)
    a.collect(); b.collect()
    assert torch.equal(a.buf["obs"], b.buf["obs"]) and a._rollout_forward_valid and not b._rollout_forward_valid
    keep = a.buf["keep"]
    assert (keep[:, 1:] == 0).any() and (keep[:, 1:] == 1).any() and (keep[:, 0] == 1).all()
    v = a.policy.views
    y, hn, cn, stash = ops.lstm_fwd(a.buf["obs"], keep, a.h0[0], a.c0[0], v["lstm.weight_ih_l0"],
                                    v["lstm.weight_hh_l0"], v["lstm.bias_ih_l0"], v["lstm.bias_hh_l0"])
    assert stash.shape == (40, 24, 6 * H)
    assert torch.allclose(a.work["y0"], y, atol=2e-6)
    assert torch.allclose(a.work["stash0"], stash, atol=2e-6)                  # all 6H columns
    hp = a.work["stash0"][..., 5 * H:]
    assert torch.equal(hp[:, 0], a.h0[0])
    assert torch.equal(hp[:, 1:], a.work["y0"][:, :-1] * keep[:, 1:, None])   # h entering step t, after the restart mask
    assert (hp[:, 1:].abs().sum(-1) > 0).any()
    a.update(); b.update()
    diff = (a.policy.flat - b.policy.flat).abs()
    assert diff.max().item() < 0.1 * 2 * 3e-5 and diff.mean().item() < 1e-7
    assert torch.allclose(a.loss_sums, b.loss_sums, rtol=1e-5)
    # trend_k = 0 leaves the slot alone
    z = mk(0)
    z.work["stash0"].fill_(-7.0)
    z.collect()
    assert z._rollout_forward_valid
    assert (z.work["stash0"][..., 5 * H:] == -7.0).all() and (z.work["stash0"][..., :5 * H] != -7.0).all()


# ---------------------------------------------------------------------------------------------- 4. greedy vs the f64 oracle
@pytest.mark.parametrize("H,k,bank_seed,pol_seed", [(128, 2, 94, 9), (64, 1, 94, 5)])
def test_fused_greedy_trend_matches_f64_oracle(ev, H, k, bank_seed, pol_seed):
    N, CAP = 21, 120
    noise = np.random.RandomState(H + k).randn(CAP, N, 2)
    bank, env = _bank_env(N, "v2.0", bank_seed, 3, trend_k=k)
    pol = _trend_policy(H, pol_seed, k)
    steps, stopped, devs, reached, gap = _oracle_lstm(pol, bank, "v2.0", N, CAP, noise, trend_k=k)
    assert gap > GAP, f"oracle's smallest top-2 logit gap {gap:g}: agreement would be luck"
    assert reached.any() and (steps == CAP).any(), (reached.sum(), steps)       # some reach the source, some time out
    blind = _trend_policy(H, pol_seed, k)
    blind.views["lstm.weight_ih_l0"][:, 6:].zero_()
    steps_blind = _oracle_lstm(blind, bank, "v2.0", N, CAP, noise, trend_k=k)[0]
    assert (steps_blind != steps).any(), "the trend channels decide nothing here"
    assert ev.fused_refusal(pol, env) is None
    got = ev.evaluate(pol, env, noise=torch.from_numpy(noise).to(DEV), max_steps=CAP, fused=True)
    _agree(got, steps, stopped, devs)
    assert np.array_equal(got["success"], devs <= ev.SUCCESS_DISTANCE_THRESHOLD)


# ---------------------------------------------------------------------------------------------- 5. chunking
@pytest.mark.parametrize("stop", [False, True])
@pytest.mark.parametrize("H,k", [(64, 1), (128, 2)])
def test_chunking_is_invisible_on_a_trend_env(H, k, stop):
    """Three calls of 40 steps give what one call of 120 gives, bit for bit: records, blob, cur_obs (6 + k wide), h, c, active
    and, with the stop rule, the window buffers."""
    from uavppo import ops
    N, CAP = 21, 120
    pol = _trend_policy(H, 2, k)
    noise = torch.from_numpy(np.random.RandomState(5).randn(N, CAP, 2)).to(DEV)
    rule = ops.make_stop_rule()
    runs = []
    for chunk in (CAP, 40):
        _, env = _bank_env(N, "v2.0", 13, 3, trend_k=k)
        env.current_radius = 200.0                        # episodes end inside the cap
        env.reset()
        cur = env.obs.clone()
        assert cur.shape == (N, 6 + k)
        g = torch.Generator().manual_seed(0)              # a carried-in state, not zero
        h = (torch.rand(N, H, generator=g) * 0.2).to(DEV)
        c = (torch.rand(N, H, generator=g) * 0.2).to(DEV)
        active = torch.ones(N, dtype=torch.uint8, device=DEV)
        win = torch.zeros(N, rule.window, 2, device=DEV)
        cnt = torch.zeros(N, dtype=torch.int32, device=DEV)
        nan = torch.zeros(1, dtype=torch.int32, device=DEV)
        recs = {"act": [], "obs": [], "pos": [], "flags": []}
        for t0 in range(0, CAP, chunk):
            r = {"act": torch.empty(N, chunk, dtype=torch.int32, device=DEV), "obs": torch.empty(N, chunk, 6 + k, device=DEV),
                 "pos": torch.empty(N, chunk, 2, device=DEV), "flags": torch.empty(N, chunk, dtype=torch.uint8, device=DEV)}
            nz = noise[:, t0:t0 + chunk].contiguous()
            if stop:
                ops.greedy_episodes_stop(env.state, N, env.cfg(), pol.flat, H, chunk, cur, h, c, active, r, rule, win, cnt,
                                         noise=nz, nan_count=nan)
            else:
                ops.greedy_episodes(env.state, N, env.cfg(), pol.flat, H, chunk, cur, h, c, active, r, noise=nz, nan_count=nan)
            for key in recs:
                recs[key].append(r[key])
        recs = {key: torch.cat(v, 1).cpu() for key, v in recs.items()}
        runs.append((recs, [env.state.cpu(), cur.cpu(), h.cpu(), c.cpu(), active.cpu(), win.cpu(), cnt.cpu(), int(nan.item())]))
    (ra, fa), (rb, fb) = runs
    for key in ra:
        assert torch.equal(ra[key], rb[key]), key
    for i, (x, y) in enumerate(zip(fa, fb)):
        assert torch.equal(x, y) if torch.is_tensor(x) else x == y, i
    flags = ra["flags"]
    assert fa[7] == 0
    ended = (flags & (9 if stop else 1)) != 0
    assert ended[:, :80].any(), "no episode ended before the last chunk: freezing across chunks went untested"
    assert (ra["obs"][..., 6:][(flags & 4) == 0] != 0).any()
    assert (ra["obs"][(flags & 4) != 0] == 0).all() and (ra["pos"][(flags & 4) != 0] == 0).all()


# ---------------------------------------------------------------------------------------------- 6. stop rule, ModelEvaluator
def _oracle_v11_trend(pol, N, cap, seed, k):
    """tests/_eval_v11_check.oracle_episodes for a procedural v1.1 env with trend channels and the env's own step noise:
    (steps, stopped, success, smallest top-2 gap, std margin, concentration margin)."""
    p = {key: v.detach().cpu().double() for key, v in pol.named_views().items()}
    H = pol.hidden
    ora = pr.ProceduralVecEnv(N, seed, "v1.1", trend_k=k)
    ora.reset()
    steps, stopped, success = [], [], []
    gap, std_margin, conc_margin = np.inf, np.inf, np.inf
    for i, e in enumerate(ora.envs):
        h = torch.zeros(1, 1, H, dtype=torch.float64)
        c = torch.zeros_like(h)
        state, traj, t, over, fired = e.obs(), [], 0, False, False
        while not over and t < cap:
            with torch.no_grad():
                _, _, logits, (h, c) = po.lstm_policy_forward(p, torch.from_numpy(state.astype(np.float64))[None, None], h, c)
            z = logits[0, 0].numpy()
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


def test_model_evaluator_runs_a_trend_policy_fused():
    """ModelEvaluator on a trend_k = 1 env: the fused run (uav_greedy_episodes_stop, TREND form) and the step-wise run give
    the same steps / stops / success -- those of the f64 oracle, whose margins make the agreement meaningful."""
    if PKG not in sys.path:
        sys.path.insert(0, PKG)
    import evaluate_model as em
    from evaluate_with_lstm import fused_refusal
    from uavppo.vec_env import VecMethaneEnv
    N, CAP, k = 21, 300, 1
    pol = _trend_policy(64, 9, k)
    env = VecMethaneEnv(N, "v1.1", DEV, trend_k=k)
    steps, stopped, success, gap, std_margin, conc_margin = _oracle_v11_trend(pol, N, CAP, env.seed, k)
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


# ---------------------------------------------------------------------------------------------- 7. refusals
def test_refusals_name_their_reason(ev):
    from uavppo import ops
    from uavppo.policy import MLPActorCritic
    from uavppo.vec_env import VecMethaneEnv
    N = 16
    env2, env1, env0 = (VecMethaneEnv(N, "v2.0", DEV, trend_k=k) for k in (2, 1, 0))
    # obs_dim and 6 + trend_k disagree, either way: both numbers and trend_k are named
    why = ev.fused_refusal(_lstm_policy(64, 1), env2)
    assert why is not None and "obs_dim is 6" in why and "8 features" in why and "trend_k = 2" in why
    with pytest.raises(RuntimeError, match="obs_dim is 6.*8 features.*trend_k = 2"):
        ev.evaluate(_lstm_policy(64, 1), env2, max_steps=5, fused=True)
    why = ev.fused_refusal(_lstm_policy(64, 1, obs_dim=7), env0)
    assert why is not None and "obs_dim is 7" in why and "6 features" in why and "trend_k = 0" in why
    assert ev.fused_refusal(_lstm_policy(64, 1, obs_dim=8), env2) is None
    assert ev.fused_refusal(_lstm_policy(128, 1, obs_dim=7), env1) is None
    # shapes the kernel does not cover, on a trend env: the shape and trend_k
    why = ev.fused_refusal(_lstm_policy(96, 1, obs_dim=7), env1)
    assert why is not None and "hidden 96" in why and "trend_k = 1" in why
    # the MLP has 6 inputs
    mlp = MLPActorCritic(6, 5, device=DEV, seed=1)
    why = ev.fused_refusal(mlp, env1)
    assert why is not None and "trend_k = 1" in why and "MLP" in why
    # the C ABI: MLP policy with trend_k = 1, and h = 96, refused before anything runs
    env1.reset()
    recs = {"act": torch.empty(N, 4, dtype=torch.int32, device=DEV), "obs": torch.empty(N, 4, 7, device=DEV),
            "pos": torch.empty(N, 4, 2, device=DEV), "flags": torch.full((N, 4), 0xA5, dtype=torch.uint8, device=DEV)}
    act = torch.ones(N, dtype=torch.uint8, device=DEV)
    obs_before = env1.obs.clone()
    with pytest.raises(RuntimeError, match=r"uav_greedy_episodes: trend_k=1 unsupported \(the fused MLP kernels take 6"):
        ops.greedy_episodes(env1.state, N, env1.cfg(), mlp.flat, 0, 4, env1.obs, None, None, act, recs)
    cnt = torch.zeros(N, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match=r"uav_greedy_episodes_stop: trend_k=1 unsupported \(the fused MLP kernels take 6"):
        ops.greedy_episodes_stop(env1.state, N, env1.cfg(), mlp.flat, 0, 4, env1.obs, None, None, act, recs, ops.make_stop_rule(),
                                 torch.zeros(N, 10, 2, device=DEV), cnt)
    h = torch.zeros(N, 96, device=DEV)
    with pytest.raises(RuntimeError, match="hidden=96"):
        ops.greedy_episodes(env1.state, N, env1.cfg(), _lstm_policy(96, 1, obs_dim=7).flat, 96, 4, env1.obs, h, h.clone(), act, recs)
    # a 6-wide record buffer on a trend env is caught by the wrapper's shape check
    with pytest.raises(RuntimeError, match="obs"):
        ops.greedy_episodes(env1.state, N, env1.cfg(), _lstm_policy(64, 1, obs_dim=7).flat, 64, 4, env1.obs, h[:, :64].contiguous(),
                            h[:, :64].contiguous(), act, dict(recs, obs=torch.empty(N, 4, 6, device=DEV)))
    assert (recs["flags"].cpu() == 0xA5).all() and int(cnt.sum()) == 0 and torch.equal(env1.obs, obs_before)   # nothing ran
    assert (act == 1).all()


# ---------------------------------------------------------------------------------------------- 8. generate_expert_data
def test_generate_expert_data_of_a_trend_policy(monkeypatch):
    """An h = 64, obs_dim = 7 policy: states of width 7 from the fused kernel, equal to the pairs the step-wise loop cuts for
    the same policy and environment (oracle gap of this case 1.3e-3; two episodes end inside the cap)."""
    if PKG not in sys.path:
        sys.path.insert(0, PKG)
    import generate_expert_data as ged
    from uavppo.vec_env import VecMethaneEnv
    N, steps, seed = 12, 120, 5
    pol = _trend_policy(64, 5, 1)
    assert ged.fused_refusal(pol, VecMethaneEnv(N, "v2.0", DEV, seed=seed, trend_k=1)) is None
    states, actions = ged.generate_expert_data(pol, num_episodes=N, variant="v2.0", seed=seed, max_steps=steps, out=None)
    assert states.shape[1] == 7 and states.dtype == np.float32 and actions.dtype == np.int64
    assert 0 < len(actions) < N * steps and actions.min() >= 0 and actions.max() < 5
    assert (states[:, 6] != 0).any()
    monkeypatch.setattr(ged, "fused_refusal", lambda policy, env: "step-wise wanted")
    s2, a2 = ged.generate_expert_data(pol, num_episodes=N, variant="v2.0", seed=seed, max_steps=steps, out=None)
    assert np.array_equal(states, s2) and np.array_equal(actions, a2)
