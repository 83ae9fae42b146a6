"""Greedy evaluation of policy objects (evaluate_with_lstm.evaluate) and the fused greedy-episode kernels behind it
(uav_greedy_episodes: rollout_lstm_kernel / rollout_mlp_kernel in their GREEDY form) against f64 oracle episodes built from
oracle.ppo_oracle and OracleVecEnv, the step-wise path, and themselves under chunking.  -m gpu."""
import os
import re
import sys

import numpy as np
import pytest
import torch

from oracle import eval_oracle as eo
from oracle import ppo_oracle as po
from oracle.env_oracle import FieldBank, OracleVecEnv

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "uav-wrf-les-ppo-lstm_amd")
# decisions in f32 arithmetic (logit errors ~1e-5 at these scales) equal the f64 oracle's when every top-2 logit gap the
# oracle met is above this
GAP = 1e-4


@pytest.fixture(scope="module")
def ev():
    if PKG not in sys.path:
        sys.path.insert(0, PKG)
    import evaluate_with_lstm as m
    return m


def _lstm_policy(H, seed, layers=1, obs_dim=6, scale=400.0, bias=None):
    from uavppo.policy import LSTMActorCritic
    pol = LSTMActorCritic(obs_dim, H, layers, device=DEV, seed=seed)
    pol.views["head.weight"][:5].mul_(scale)              # a decisive greedy policy (actor rows of gain 0.01 otherwise)
    if bias is not None:
        pol.views["head.bias"][:5].copy_(torch.tensor(bias))
    return pol


def _p64(pol):
    return {k: v.detach().cpu().double() for k, v in pol.named_views().items()}


def _oracle_lstm(pol, bank, variant, N, cap, noise, trend_k=0, stop=None):
    """One f64 episode per env: (h, c) from zero, argmax of the logits; stop() -> rule(traj, t) -> bool makes one env's
    controller.
    Returns steps, stopped, deviations, reached, smallest top-2 logit gap."""
    p = _p64(pol)
    L, H = pol.num_layers, pol.hidden
    ora = OracleVecEnv(N, bank, variant, radius=50.0, trend_k=trend_k)
    ora.reset()
    steps, stopped, devs, reached, gap = [], [], [], [], np.inf
    for i, e in enumerate(ora.envs):
        h = torch.zeros(L, 1, H, dtype=torch.float64)
        c = torch.zeros_like(h)
        state, traj, t, done, st, rc = e.obs(), [], 0, False, False, False
        rule = stop() if stop is not None else None
        while not done and t < cap:
            x = torch.from_numpy(state.astype(np.float64))[None, None]
            with torch.no_grad():
                _, _, logits, (h, c) = po.lstm_policy_forward(p, x, h, c)
            z = logits[0, 0]
            top = torch.topk(z, 2).values
            gap = min(gap, float(top[0] - top[1]))
            state, _, done, rc, _ = e.step(int(torch.argmax(z)), noise[t, i])
            traj.append(float(state[2]) * 100.0)
            t += 1
            if rule is not None and rule(traj, t):
                st, done = True, True
        steps.append(t)
        stopped.append(st)
        reached.append(rc)
        devs.append(float(np.linalg.norm(np.asarray(e.pos, np.float64) - np.asarray(e.source, np.float64))))
    return np.asarray(steps), np.asarray(stopped), np.asarray(devs), np.asarray(reached), gap


def _bank_env(N, variant, seed, env_seed, trend_k=0):
    from uavppo.vec_env import VecMethaneEnv
    bank = FieldBank.from_seed(N, variant, seed=seed)
    env = VecMethaneEnv(N, variant, DEV, seed=env_seed, bank=bank.interleaved(), bank_sources=bank.sources, trend_k=trend_k)
    return bank, env


def _agree(got, want_steps, want_stopped, want_devs):
    assert np.array_equal(got["steps"], want_steps), (got["steps"], want_steps)
    assert np.array_equal(got["stopped_early"], want_stopped)
    assert np.allclose(got["deviations"], want_devs, atol=2e-3)


def _equal(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), k


TOWARDS = [0.0, 2.0, -5.0, 2.0, -5.0]                    # head bias: +x / +y from the corner, so some episodes reach the source


# ---------------------------------------------------------------------------------------------- 1. fused LSTM vs oracle
@pytest.mark.parametrize("H", [64, 128])
def test_fused_lstm_matches_f64_oracle(ev, H):
    N, CAP = 37, 200
    noise = np.random.RandomState(H).randn(CAP, N, 2)
    bank, env = _bank_env(N, "v2.0", 94 if H == 64 else 158, 3)
    pol = _lstm_policy(H, seed=6 if H == 64 else 5, bias=TOWARDS)
    steps, stopped, devs, reached, gap = _oracle_lstm(pol, bank, "v2.0", N, CAP, noise)
    assert gap > GAP, f"oracle's smallest top-2 logit gap {gap:g}: agreement would be luck"
    assert reached.any() and (steps == CAP).any(), (reached.sum(), steps)       # some reach the source, some time out
    got = ev.evaluate(pol, env, noise=torch.from_numpy(noise).to(DEV), max_steps=CAP, fused=True)
    _agree(got, steps, stopped, devs)
    assert np.array_equal(got["success"], devs <= ev.SUCCESS_DISTANCE_THRESHOLD)


# ---------------------------------------------------------------------------------------------- 2. with each controller
def _threshold_controller(ev, N):
    pred = ev.ConcentrationThresholdPredictor(hidden_size=64, device=DEV, seed=4)
    pred.fc["fc.4.bias"].fill_(18.0)                      # thresholds inside the plume's concentration range
    pred.fc["fc.4.weight"].mul_(6.0)
    return pred, ev.ThresholdController(pred, (0.0, 100.0), N, device=DEV)


def _peak_stop(ev):
    pred = ev.PeakAndStopPredictor(device=DEV, seed=6)
    pred.heads_w[1].mul_(12.0)                            # a decisive stop head
    return pred


@pytest.mark.parametrize("kind", ["mlp", "lstm"])
@pytest.mark.parametrize("rule", ["v2.0", "v2.1"])
def test_fused_with_controller_equals_callable_path(ev, kind, rule):
    """Same env seed, same decisions: the fused object path and the existing callable path give bit-identical metrics."""
    from uavppo.policy import MLPActorCritic
    if kind == "mlp":
        N, LIM, bseed = 24, 150, 9
        pol = MLPActorCritic(6, 5, device=DEV, seed=8)
        pol.views["head.weight"][:5].mul_(40.0)
    else:
        N, LIM, bseed = 37, 200, 94
        pol = _lstm_policy(64, seed=6, bias=TOWARDS)
    noise = torch.from_numpy(np.random.RandomState(7).randn(LIM, N, 2)).to(DEV)
    results = []
    for path in ("callable", "fused"):
        bank, env = _bank_env(N, rule, bseed, 3)
        ctl, peak = None, None
        if rule == "v2.0":
            _, ctl = _threshold_controller(ev, N)
        else:
            peak = _peak_stop(ev)
        if path == "fused":
            results.append(ev.evaluate(pol, env, ctl, peak_stop=peak, noise=noise, max_steps=LIM, fused=True, chunk=23))
        elif kind == "mlp":
            results.append(ev.evaluate(lambda o: pol.heads(o.contiguous())[:, :5], env, ctl, peak_stop=peak, noise=noise,
                                       max_steps=LIM))
        else:
            h, c = pol.zero_state(N)
            results.append(ev.evaluate(lambda o: pol.step(o, h, c)[:, :5], env, ctl, peak_stop=peak, noise=noise, max_steps=LIM))
    _equal(results[0], results[1])
    got = results[1]
    assert got["stopped_early"].any() or np.ptp(got["steps"]) > 0


def test_fused_lstm_with_threshold_controller_matches_oracle(ev):
    N, LIM = 37, 200                                      # test 1's h = 64 scenario, now with the controller
    noise = np.random.RandomState(64).randn(LIM, N, 2)
    bank, env = _bank_env(N, "v2.0", 94, 3)
    pol = _lstm_policy(64, seed=6, bias=TOWARDS)
    pred, ctl = _threshold_controller(ev, N)
    onet = eo.ThresholdPredictorOracle({k: v.detach().cpu().numpy() for k, v in pred.state_dict().items()})

    def stop():                                           # evaluate_with_lstm.py:87-93 for one env's episode
        o = eo.ThresholdControllerOracle(onet, np.array((0.0, 100.0)))

        def rule(traj, t):
            if t % 10 == 0:
                o.update_threshold(traj)
            return o.should_stop(traj[-1], t)
        return rule

    steps, stopped, devs, _, gap = _oracle_lstm(pol, bank, "v2.0", N, LIM, noise, stop=stop)
    assert gap > GAP, gap
    got = ev.evaluate(pol, env, ctl, noise=torch.from_numpy(noise).to(DEV), max_steps=LIM, fused=True)
    _agree(got, steps, stopped, devs)
    assert 0 < stopped.sum() < N or np.ptp(steps) > 0


# ---------------------------------------------------------------------------------------------- 3. chunk invariance
@pytest.mark.parametrize("kind", ["lstm64", "lstm128", "mlp"])
def test_chunking_is_invisible(ev, kind):
    from uavppo import ops
    from uavppo.policy import MLPActorCritic
    N, CAP = 40, 120
    if kind == "mlp":
        pol, H = MLPActorCritic(6, 5, device=DEV, seed=3), 0
        pol.views["head.weight"][:5].mul_(40.0)
        pol.views["head.bias"][:5].copy_(torch.tensor(TOWARDS))
    else:
        H = int(kind[4:])
        pol = _lstm_policy(H, seed=2, bias=TOWARDS)
    noise = torch.from_numpy(np.random.RandomState(5).randn(N, CAP, 2)).to(DEV)
    frozen = torch.arange(N, device=DEV) % 5 == 3         # these come in inactive
    runs = []
    for chunk in (1, 7, 64, CAP):
        _, env = _bank_env(N, "v2.0", 13, 3)
        env.current_radius = 200.0                        # episodes end inside the cap: freezing gets tested
        env.reset()
        before = [t.clone() for t in env.peek()]
        cur = env.obs.clone()
        g = torch.Generator().manual_seed(0)                             # a carried-in state, not zero
        h = (torch.rand(N, H, generator=g) * 0.2).to(DEV) if H else None
        c = (torch.rand(N, H, generator=g) * 0.2).to(DEV) if H else None
        h0 = None if h is None else h.clone()
        c0 = None if c is None else c.clone()
        active = (~frozen).to(torch.uint8)
        nan = torch.zeros(1, dtype=torch.int32, device=DEV)
        recs = {"act": [], "obs": [], "pos": [], "flags": []}
        n_ended_checked = 0
        for t0 in range(0, CAP, chunk):
            k = min(chunk, CAP - t0)
            r = {"act": torch.empty(N, k, dtype=torch.int32, device=DEV), "obs": torch.empty(N, k, 6, device=DEV),
                 "pos": torch.empty(N, k, 2, device=DEV), "flags": torch.empty(N, k, dtype=torch.uint8, device=DEV)}
            # an env inactive before a chunk (ended in an earlier one, or passed in inactive) is untouched by it: its peek view,
            # observation, h and c
            ended = active == 0
            peek_before = [t.clone() for t in env.peek()]
            cur_before = cur.clone()
            hc_before = None if h is None else (h.clone(), c.clone())
            ops.greedy_episodes(env.state, N, env.cfg(), pol.flat, H, k, cur, h, c, active, r,
                                noise=noise[:, t0:t0 + k].contiguous(), nan_count=nan)
            for b, a in zip(peek_before, env.peek()):
                assert torch.equal(b[ended], a[ended]), t0
            assert torch.equal(cur_before[ended], cur[ended])
            if H:
                assert torch.equal(hc_before[0][ended], h[ended]) and torch.equal(hc_before[1][ended], c[ended])
            assert (r["flags"][ended] == 4).all()
            n_ended_checked += int((ended & ~frozen).sum())
            for key in recs:
                recs[key].append(r[key])
        recs = {key: torch.cat(v, 1).cpu() for key, v in recs.items()}
        after = env.peek()
        # envs passed in inactive: blob untouched (peek), records "not stepped", h / c / cur_obs untouched
        for b, a in zip(before, after):
            assert torch.equal(b[frozen], a[frozen])
        assert (recs["flags"][frozen.cpu()] == 4).all() and (recs["act"][frozen.cpu()] == -1).all()
        if H:
            assert torch.equal(h[frozen], h0[frozen]) and torch.equal(c[frozen], c0[frozen])
        runs.append((recs, env.state.clone().cpu(), cur.cpu(), None if h is None else h.cpu(), None if c is None else c.cpu(),
                     active.cpu(), int(nan.item())))
        if chunk == 7:
            assert n_ended_checked > 0, "no episode ended before a later chunk: freezing across chunks went untested"
            flags = recs["flags"]
            done_at = ((flags & 1) != 0).int().argmax(1)
            ended = ((flags & 1) != 0).any(1)
            assert ended.any(), "no episode ended: the chunk test would not test freezing"
            stepped = (flags & 4) == 0
            for n in torch.nonzero(ended).reshape(-1).tolist():
                assert stepped[n, :done_at[n] + 1].all() and not stepped[n, done_at[n] + 1:].any()
    ref = runs[0]
    for r in runs[1:]:
        for a, b in zip(ref[0].values(), r[0].values()):
            assert torch.equal(a, b)
        for a, b in zip(ref[1:], r[1:]):
            assert (a is None and b is None) or (torch.equal(a, b) if torch.is_tensor(a) else a == b)
    assert ref[6] == 0
    assert (ref[5][~frozen.cpu()] == 0).any()                                            # some episodes ended


def test_chunk_size_does_not_change_evaluate(ev):
    N, LIM = 30, 140
    noise = torch.from_numpy(np.random.RandomState(3).randn(LIM, N, 2)).to(DEV)
    pol = _lstm_policy(64, seed=4)
    outs = []
    for chunk in (1, 7, 64, LIM):
        _, env = _bank_env(N, "v2.0", 15, 3)
        _, ctl = _threshold_controller(ev, N)
        outs.append(ev.evaluate(pol, env, ctl, noise=noise, max_steps=LIM, fused=True, chunk=chunk))
    for o in outs[1:]:
        _equal(outs[0], o)


# ---------------------------------------------------------------------------------------------- 4. fall-backs
@pytest.mark.parametrize("case", ["2x64", "256x2_trend2", "wide"])
def test_fallbacks_match_oracle_and_refuse_fused(ev, case):
    from uavppo import ops
    N, CAP = (6, 40) if case == "256x2_trend2" else (16, 120)
    trend_k = 2 if case == "256x2_trend2" else 0
    noise = np.random.RandomState(8).randn(CAP, N, 2)
    bank, env = _bank_env(N, "v2.0", 17, 3, trend_k=trend_k)
    if case == "2x64":
        pol, why = _lstm_policy(64, seed=3, layers=2), "2 layer"
    elif case == "256x2_trend2":
        pol, why = _lstm_policy(256, seed=4, layers=2, obs_dim=8), "trend_k = 2"
    else:
        pol, why = _lstm_policy(128, seed=8), "bf16x6"
    steps, stopped, devs, _, gap = _oracle_lstm(pol, bank, "v2.0", N, CAP, noise, trend_k=trend_k)
    assert gap > GAP, gap
    nz = torch.from_numpy(noise).to(DEV)
    with ops.lstm_arith("bf16x6" if case == "wide" else "fp16x3"):
        with pytest.raises(RuntimeError, match=why):
            ev.evaluate(pol, env, noise=nz, max_steps=CAP, fused=True)
        assert ev.fused_refusal(pol, env) is not None
        got = ev.evaluate(pol, env, noise=nz, max_steps=CAP)
    _agree(got, steps, stopped, devs)


def test_fused_refuses_out_of_range_parameters_and_c_abi_names_its_reasons(ev):
    from uavppo import ops
    N = 16
    _, env = _bank_env(N, "v2.0", 19, 3)
    pol = _lstm_policy(64, seed=3)
    pol.flat[7] = 40000.0                                 # beyond RANGE_LIMITS[0]
    with pytest.raises(RuntimeError, match=re.escape("max |param| = 40000 is not below 32752")):
        ev.evaluate(pol, env, max_steps=10, fused=True)
    env.reset()
    recs = {"act": torch.empty(N, 4, dtype=torch.int32, device=DEV), "obs": torch.empty(N, 4, 6, device=DEV),
            "pos": torch.empty(N, 4, 2, device=DEV), "flags": torch.empty(N, 4, dtype=torch.uint8, device=DEV)}
    act = torch.ones(N, dtype=torch.uint8, device=DEV)
    h = torch.zeros(N, 96, device=DEV)
    with pytest.raises(RuntimeError, match="hidden=96"):
        ops.greedy_episodes(env.state, N, env.cfg(), pol.flat, 96, 4, env.obs, h, h.clone(), act, recs)
    with ops.lstm_arith("f32_mfma"):
        with pytest.raises(RuntimeError, match="fp16x3"):
            ops.greedy_episodes(env.state, N, env.cfg(), pol.flat, 64, 4, env.obs, h[:, :64].contiguous(),
                                h[:, :64].contiguous(), act, recs)


# ---------------------------------------------------------------------------------------------- 5. NaN
@pytest.mark.parametrize("kind", ["lstm", "mlp"])
@pytest.mark.parametrize("fused", [True, False])
def test_nan_parameters_raise(ev, kind, fused):
    from uavppo.policy import MLPActorCritic
    _, env = _bank_env(16, "v2.0", 23, 3)
    pol = _lstm_policy(64, seed=1) if kind == "lstm" else MLPActorCritic(6, 5, device=DEV, seed=1)
    pol.flat[3] = float("nan")
    with pytest.raises(RuntimeError, match="NaN in probs"):
        ev.evaluate(pol, env, max_steps=20, fused=fused)


# ---------------------------------------------------------------------------------------------- 6. main(policy="lstm")
def test_main_evaluates_a_vectorised_trainer_checkpoint(ev, tmp_path, monkeypatch):
    import importlib.util
    from uavppo.policy import LSTMActorCritic
    spec = importlib.util.spec_from_file_location("train_ppo20", os.path.join(PKG, "train_ppo2.0.py"))
    tp = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tp)
    cpu = LSTMActorCritic(6, 64, 1, device="cpu", seed=11)        # a CPU-built state_dict
    model_dir = tmp_path / "model"
    tp._save(cpu.state_dict(), [], None, str(model_dir / "ppo_successful_models.pth"))
    pred = ev.ConcentrationThresholdPredictor(device="cpu")
    torch.save(pred.state_dict(), str(model_dir / "lstm_threshold_predictor.pth"))
    np.save(str(model_dir / "scaler_params.npy"), np.array([0.0, 100.0]))
    loaded = ev.load_lstm_policy(str(model_dir / "ppo_successful_models.pth"), DEV)
    assert (loaded.obs_dim, loaded.hidden, loaded.num_layers, loaded.n_act) == (6, 64, 1, 5)
    assert torch.equal(loaded.flat.cpu(), cpu.flat)
    monkeypatch.chdir(tmp_path)
    m = ev.main(num_envs=32, model_dir=str(model_dir), device=DEV, policy="lstm")
    assert m is not None and m["steps"].shape == (32,) and (m["steps"] >= 1).all()
    assert os.path.exists(tmp_path / "results" / "validation_metrics.npz")


# ---------------------------------------------------------------------------------------------- 7. dispatch
@pytest.mark.parametrize("rule", [None, "v2.0"])
def test_ppo_actor_critic_is_evaluated_as_a_policy_object(ev, rule):
    """model.PPOActorCritic is an nn.Module (callable), yet evaluate() takes it as a policy object: fused and step-wise runs
    equal the MLPActorCritic and callable-path metrics bit for bit."""
    from uavppo.policy import MLPActorCritic
    from model import PPOActorCritic
    N, LIM = 24, 150
    core = MLPActorCritic(6, 5, device=DEV, seed=8)
    core.views["head.weight"][:5].mul_(40.0)
    ppo = PPOActorCritic(6, 5, device=DEV)
    ppo.core.load_state_dict(core.state_dict())
    noise = torch.from_numpy(np.random.RandomState(7).randn(LIM, N, 2)).to(DEV)
    outs = []
    for pol, kw in ((lambda o: core.heads(o.contiguous())[:, :5], {}), (ppo, {"fused": True}), (ppo, {"fused": False}),
                    (core, {"fused": True})):
        _, env = _bank_env(N, "v2.0", 9, 3)
        ctl = _threshold_controller(ev, N)[1] if rule else None
        outs.append(ev.evaluate(pol, env, ctl, noise=noise, max_steps=LIM, **kw))
    for o in outs[1:]:
        _equal(outs[0], o)


def test_callable_refuses_fused_and_chunk(ev):
    _, env = _bank_env(8, "v2.0", 9, 3)
    core = _lstm_policy(64, seed=1)
    with pytest.raises(RuntimeError, match="policy_probs function has no fused kernel"):
        ev.evaluate(lambda o: o[:, :5], env, max_steps=5, fused=True)
    with pytest.raises(ValueError, match="chunk"):
        ev.evaluate(lambda o: o[:, :5], env, max_steps=5, chunk=4)
    with pytest.raises(TypeError, match="expected a callable"):
        ev.evaluate(object(), env, max_steps=5)
    assert ev.evaluate(core, env, max_steps=5)["steps"].shape == (8,)


def test_out_of_range_policy_steps_in_bf16x6(ev):
    """fused=None with max |param| beyond RANGE_LIMITS: the step-wise path runs the policy's calls in bf16x6 (as the trainer
    switches) and leaves the handle in its own mode; the result equals a step-wise run under an explicit bf16x6 handle."""
    from uavppo import ops
    N, LIM = 16, 60
    pol = _lstm_policy(64, seed=3)
    pol.flat[7] = 40000.0
    modes = []
    step = pol.step

    def spy(*a, **k):
        modes.append(ops.get_lstm_arith())
        return step(*a, **k)

    noise = torch.from_numpy(np.random.RandomState(2).randn(LIM, N, 2)).to(DEV)
    assert ops.get_lstm_arith() == "fp16x3"
    pol.step = spy
    _, env = _bank_env(N, "v2.0", 19, 3)
    got = ev.evaluate(pol, env, noise=noise, max_steps=LIM)
    del pol.step
    assert modes and set(modes) == {"bf16x6"} and ops.get_lstm_arith() == "fp16x3"
    _, env = _bank_env(N, "v2.0", 19, 3)
    with ops.lstm_arith("bf16x6"):
        want = ev.evaluate(pol, env, noise=noise, max_steps=LIM, fused=False)
    _equal(got, want)
