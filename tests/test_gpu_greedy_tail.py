"""uav_greedy_tail (csrc/greedy_tail.hip) and the tail route of greedy evaluation built on it (uavppo.greedy.GreedyRun(tail=True),
evaluate(tail=), ModelEvaluator.run_evaluation(tail=), generate_expert_data(tail=)).  Everything here is an IDENTITY: the kernel
against the calls it replaces (gemm_rows + argmax + env_step + stop_stability) on twin envs, the route against the step-wise loop.
No tolerance anywhere: torch.equal / np.array_equal.  -m gpu."""
import os
import sys

import numpy as np
import pytest
import torch

from oracle.env_oracle import FieldBank

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "uav-wrf-les-ppo-lstm_amd")
LSTM_GAIN = 8.0                                          # on the LSTM weights: actions that depend on the observation AND on (h, c)
F32 = torch.float32


@pytest.fixture(scope="module")
def ev():
    if PKG not in sys.path:
        sys.path.insert(0, PKG)
    import evaluate_with_lstm as m
    return m


@pytest.fixture(scope="module")
def em():
    if PKG not in sys.path:
        sys.path.insert(0, PKG)
    import evaluate_model as m
    return m


def _lstm_policy(H, seed, layers=1, obs_dim=6, scale=400.0):
    """A greedy policy whose actions vary: no head bias, LSTM weights x LSTM_GAIN (still far inside the fp16-split range).  On the
    f64 oracle over the route tests' envs each of the four shapes used below takes 4 or 5 different actions, and evaluated from
    zero state at every step it takes other actions and ends its episodes at other steps; the tests assert both on the device."""
    from uavppo.policy import LSTMActorCritic
    pol = LSTMActorCritic(obs_dim, H, layers, device=DEV, seed=seed)
    for k, v in pol.views.items():
        if k.startswith("lstm.weight"):
            v.mul_(LSTM_GAIN)
    pol.views["head.weight"][:5].mul_(scale)              # decisive logits (actor rows of gain 0.01 otherwise)
    return pol


_BANKS = {}


def _bank_env(N, variant, seed, trend_k=0, radius=None):
    """A VecMethaneEnv over a materialised bank (one field per env); the bank is built and uploaded once per (N, variant, seed)."""
    from uavppo.vec_env import VecMethaneEnv
    key = (N, variant, seed)
    if key not in _BANKS:
        bank = FieldBank.from_seed(N, variant, seed=seed)
        _BANKS[key] = (torch.from_numpy(bank.interleaved()).to(DEV), torch.from_numpy(bank.sources).to(DEV))
    fields, src = _BANKS[key]
    env = VecMethaneEnv(N, variant, DEV, seed=3, bank=fields, bank_sources=src, trend_k=trend_k)
    if radius is not None:
        env.current_radius = float(radius)
    return env


def _pattern_recs(N, steps, D):
    return {"act": torch.full((N, steps), 77, dtype=torch.int32, device=DEV), "obs": torch.full((N, steps, D), 7.5, device=DEV),
            "pos": torch.full((N, steps, 2), -3.25, device=DEV), "flags": torch.full((N, steps), 0xAA, dtype=torch.uint8, device=DEV)}


def _outside_t_intact(recs, steps, t):
    other = [i for i in range(steps) if i != t]
    pat = _pattern_recs(recs["act"].shape[0], steps, recs["obs"].shape[2])
    for k in recs:
        assert torch.equal(recs[k][:, other], pat[k][:, other]), k


def _twin_envs(n_twins, N, variant, seed, trend_k, gen):
    """n_twins procedural envs in the same state: reset, then two steps of the same random actions and noise"""
    from uavppo.vec_env import VecMethaneEnv
    envs = [VecMethaneEnv(N, variant, DEV, seed=seed, trend_k=trend_k) for _ in range(n_twins)]
    for e in envs:
        e.reset()
    for _ in range(2):
        act = torch.randint(0, 5, (N,), generator=gen).to(torch.int32).to(DEV)
        nz = torch.randn(N, 2, generator=gen, dtype=torch.float64).to(DEV)
        for e in envs:
            e.step(act, nz)
    for e in envs[1:]:
        assert torch.equal(e.state, envs[0].state) and torch.equal(e.obs, envs[0].obs)
    return envs


# ---------------------------------------------------------------------------------------------- 1. the kernel, bit for bit
@pytest.mark.parametrize("variant", ["v2.0", "v2.1"])
@pytest.mark.parametrize("N", [1, 3, 4, 5, 16, 17, 37])
def test_tail_equals_the_calls_it_replaces(N, variant):
    """One uav_greedy_tail against gemm_rows + torch.argmax + env_step on a twin env in the same state (a second twin with a
    radius nothing reaches gives agent_pos after the move for the envs whose twin auto-reset).  A radius of 350 px ends about half
    of the episodes on the tested step.  About a third of the envs come in inactive, one of them with NaN logits."""
    from uavppo import ops
    gen = torch.Generator().manual_seed(1000 * N + (variant == "v2.1"))
    seen_done = seen_live = 0
    for H in (64, 128, 256):
        for trend_k in (0, 1, 2):
            for steps, t in ((1, 0), (7, 0), (7, 6)):
                D = 6 + trend_k
                ldy = H + 12 if (H, trend_k) == (128, 1) else H               # rows of y further apart than `hidden`, once
                env, twin, far = _twin_envs(3, N, variant, 11 + trend_k, trend_k, gen)
                env.current_radius = twin.current_radius = 350.0
                far.current_radius = 1e-3                                       # never reached: no reset, agent_pos stays readable
                y_full = torch.randn(N, ldy, generator=gen).to(DEV)
                y = y_full[:, :H]
                W = (torch.randn(6, H, generator=gen) * 0.5).to(DEV)
                b = torch.randn(6, generator=gen).to(DEV)
                noise = torch.randn(N, 2, generator=gen, dtype=torch.float64).to(DEV)
                inactive = (torch.arange(N) % 3 == 1).to(DEV)
                if bool(inactive.any()):
                    y_full[int(inactive.nonzero()[0]), 5] = float("nan")        # an inactive env's NaN logits are not counted
                active = (~inactive).to(torch.uint8)
                recs = _pattern_recs(N, steps, D)
                nan_count = torch.zeros(1, dtype=torch.int32, device=DEV)
                obs_before, peek_before = env.obs.clone(), [x.clone() for x in env.peek()]
                ops.greedy_tail(env.state, env.cfg(), y, W, b, t, env.obs, active, recs, nan_count, noise=noise)
                # ---- the calls it replaces
                heads = torch.empty(N, 6, device=DEV)
                ops.gemm_rows(y, W, b, heads)
                act = torch.argmax(heads[:, :5], dim=1).to(torch.int32)
                obs_next, _, done, _ = twin.step(act, noise)
                far.step(act, noise)
                done_b = done > 0.5
                obs_rec = torch.where(done_b[:, None], twin.term_obs, obs_next)
                on = ~inactive
                assert torch.equal(recs["act"][on, t], act[on])
                assert torch.equal(recs["obs"][on, t], obs_rec[on])
                assert torch.equal(recs["pos"][on, t], far.peek()[0][on])
                assert torch.equal(recs["flags"][on, t], twin.flags[on] & 3)
                assert torch.equal(env.obs[on], obs_rec[on])
                assert torch.equal(active.bool(), on & ~done_b)
                live = on & ~done_b                                             # a done env auto-reset on the twin, froze in the tail
                for got, want in zip(env.peek(), twin.peek()):
                    assert torch.equal(got[live], want[live])
                # ---- inactive envs: the "not stepped" record, nothing else touched
                assert bool((recs["act"][inactive, t] == -1).all()) and bool((recs["flags"][inactive, t] == 4).all())
                assert bool((recs["obs"][inactive, t] == 0).all()) and bool((recs["pos"][inactive, t] == 0).all())
                assert torch.equal(env.obs[inactive], obs_before[inactive])
                for got, want in zip(env.peek(), peek_before):
                    assert torch.equal(got[inactive], want[inactive])
                assert int(nan_count.item()) == 0
                _outside_t_intact(recs, steps, t)
                seen_done += int((on & done_b).sum())
                seen_live += int(live.sum())
    if N >= 16:
        assert seen_done > 0 and seen_live > 0, (seen_done, seen_live)


# ---------------------------------------------------------------------------------------------- 2. argmax and NaN
def test_equal_logits_pick_the_first_and_nan_logits_are_counted_per_active_env(ev):
    from uavppo import ops
    N, H = 17, 64
    gen = torch.Generator().manual_seed(5)
    (env,) = _twin_envs(1, N, "v2.0", 4, 0, gen)
    y = torch.randn(N, H, generator=gen).to(DEV)
    W = torch.zeros(6, H, device=DEV)
    b = torch.tensor([1.0, 3.0, 3.0, 0.0, 3.0, 9.0], device=DEV)          # three equal maxima: the first wins; row 5 is the critic's
    active = torch.ones(N, dtype=torch.uint8, device=DEV)
    active[2] = 0
    recs = _pattern_recs(N, 1, 6)
    nan_count = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.greedy_tail(env.state, env.cfg(), y, W, b, 0, env.obs, active, recs, nan_count)
    on = torch.ones(N, dtype=torch.bool, device=DEV)
    on[2] = False
    assert bool((recs["act"][on, 0] == 1).all()) and int(recs["act"][2, 0]) == -1 and int(nan_count.item()) == 0
    W[3, 7] = 1.0
    y[[2, 4, 9, 16], 7] = float("nan")                                      # env 2 is inactive: three are counted
    active = on.to(torch.uint8)
    ops.greedy_tail(env.state, env.cfg(), y, W, b, 0, env.obs, active, recs, nan_count)
    assert int(nan_count.item()) == 3
    with pytest.raises(RuntimeError, match="t=1"):                          # the entry point's checks
        ops.greedy_tail(env.state, env.cfg(), y, W, b, 1, env.obs, active, recs, nan_count)
    pol = _lstm_policy(64, seed=1, layers=2)
    pol.flat[3] = float("nan")
    with pytest.raises(RuntimeError, match="NaN in probs"):
        ev.evaluate(pol, _bank_env(N_R, "v2.0", 17), max_steps=20, tail=True)


# ---------------------------------------------------------------------------------------------- 3. the stop rule in the tail
@pytest.mark.parametrize("window", [1, 10])
def test_stop_rule_in_the_tail_equals_stop_stability(window):
    """25 tail steps on 17 envs (random logits, a radius of 400 px so that some episodes end by `done`), the rule's window in
    place; uav_stop_stability stepped over the recorded positions / obs[2] gives the same hits, values and window buffers."""
    from uavppo import ops
    N, H, T = 17, 64, 25
    gen = torch.Generator().manual_seed(40 + window)
    (env,) = _twin_envs(1, N, "v2.0", 6, 0, gen)
    env.current_radius = 400.0
    # window 1: a std of one sample is 0, so the concentration half decides; window 10: both halves matter
    rule = ops.make_stop_rule(window, pos_std_max=1.0 if window == 1 else 25.0, conc_min=1200.0 if window == 1 else 600.0)
    W = (torch.randn(6, H, generator=gen) * 0.5).to(DEV)
    b = torch.randn(6, generator=gen).to(DEV)
    recs = _pattern_recs(N, T, 6)
    rule_val = torch.full((N, T), 5.5, device=DEV)
    active = torch.ones(N, dtype=torch.uint8, device=DEV)
    nan_count = torch.zeros(1, dtype=torch.int32, device=DEV)
    win, cnt = torch.zeros(N, window, 2, device=DEV), torch.zeros(N, dtype=torch.int32, device=DEV)
    win_ref, cnt_ref = win.clone(), cnt.clone()
    steps_taken = torch.zeros(N, dtype=torch.int32, device=DEV)
    for t in range(T):
        y = torch.randn(N, H, generator=gen).to(DEV)
        noise = torch.randn(N, 2, generator=gen, dtype=torch.float64).to(DEV)
        before = active.clone()
        ops.greedy_tail(env.state, env.cfg(), y, W, b, t, env.obs, active, recs, nan_count, noise=noise, rule=rule, stop_win=win,
                        stop_cnt=cnt, rule_val=rule_val)
        hit, val = ops.stop_stability(rule, recs["pos"][:, t].contiguous(), recs["obs"][:, t, 2], win_ref, cnt_ref, active=before)
        on = before.bool()
        assert torch.equal((recs["flags"][:, t] & 8) != 0, (hit != 0) & on), t
        assert torch.equal(rule_val[:, t].view(torch.int32), val.view(torch.int32)), t        # the bits, NaN included
        assert torch.equal(win, win_ref) and torch.equal(cnt, cnt_ref), t
        ended = (recs["flags"][:, t] & 9) != 0
        assert torch.equal(active.bool(), on & ~ended), t
        assert bool((recs["flags"][~on, t] == 4).all()) and bool((recs["act"][~on, t] == -1).all())
        steps_taken += on.to(torch.int32)
    hit_any, done_any = ((recs["flags"] & 8) != 0).any(1), ((recs["flags"] & 1) != 0).any(1)
    print(f"window {window}: {int(hit_any.sum())} envs hit, {int(done_any.sum())} done, {int(active.sum())} still active")
    judged = (rule_val == rule_val) & ((recs["flags"] & 4) == 0)               # stepped with a full window
    assert bool(hit_any.any()) and bool((judged & ((recs["flags"] & 8) == 0)).any())     # the rule fired, and it declined
    # never stepped again after a hit (or done): the env's own step counter stands where its last record left it
    (env2,) = _twin_envs(1, N, "v2.0", 6, 0, torch.Generator().manual_seed(40 + window))
    assert torch.equal(env.peek()[2] - env2.peek()[2], steps_taken)
    assert int(nan_count.item()) == 0


# ---------------------------------------------------------------------------------------------- 4. route identity
N_R, CAP = 24, 40
POLICIES = {
    "256x1": dict(H=256, layers=1, seed=4),
    "256x2_trend2": dict(H=256, layers=2, seed=4, obs_dim=8),
    "64x2": dict(H=64, layers=2, seed=3),
    "128x1_bf16x6": dict(H=128, layers=1, seed=8),
    "128x1_out_of_range": dict(H=128, layers=1, seed=8),
}


def _route_case(name):
    """(policy, fresh-env factory, noise, arithmetic mode of the handle) of a route-identity case"""
    kw = dict(POLICIES[name])
    pol = _lstm_policy(kw.pop("H"), **kw)
    if name == "128x1_out_of_range":
        pol.flat[7] = 40000.0                                 # beyond the fp16-split range limit: the policy's calls run in bf16x6
    trend_k = pol.obs_dim - 6
    variant = "v2.1" if trend_k else "v2.0"
    noise = torch.from_numpy(np.random.RandomState(8).randn(CAP, N_R, 2)).to(DEV)
    return pol, (lambda: _bank_env(N_R, variant, 17, trend_k, radius=200.0)), noise, "bf16x6" if name == "128x1_bf16x6" else "fp16x3"


def _equal(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), (k, a[k], b[k])


@pytest.mark.parametrize("name", list(POLICIES))
def test_layers_of_the_tail_backend_equal_lstm_actor_critic_step(name):
    """The top layer's y of GreedyRun(tail=True).layers_step() against LSTMActorCritic.step(want_heads=False) with its own carried
    (h, c), over 40 consecutive env steps (the stepper backend begins new segments at steps 16 and 32), and the logits of
    uav_gemm_f32 on both: torch.equal at every step.  The y of a run that forgets its state differs."""
    from uavppo import ops
    from uavppo.greedy import GreedyRun
    pol, fresh_env, noise, mode = _route_case(name)
    with ops.lstm_arith(mode):
        env = fresh_env()
        env.reset()
        run = GreedyRun("lstm", pol, env, tail=True)
        assert (run.steppers is not None) == name.startswith("256")
        h, c = pol.zero_state(N_R)
        work, recs, differs_from_stateless = {}, ops.greedy_recs(N_R, CAP, env.obs_dim, DEV), 0
        for t in range(CAP):
            with ops.lstm_arith("bf16x6") if name == "128x1_out_of_range" else ops.lstm_arith(mode):
                want = pol.step(env.obs, h, c, work=work, want_heads=False).reshape(N_R, pol.hidden).clone()
                z0 = pol.zero_state(N_R)
                stateless = pol.step(env.obs, z0[0], z0[1], want_heads=False).reshape(N_R, pol.hidden)
            y = run.layers_step()
            assert torch.equal(y.reshape(N_R, pol.hidden), want), t
            differs_from_stateless += int(t > 0 and not torch.equal(want, stateless))
            v = pol.views
            heads = torch.empty(N_R, 6, device=DEV)
            ops.gemm_rows(y.reshape(N_R, pol.hidden), v["head.weight"], v["head.bias"], heads)
            assert torch.equal(heads, ops.gemm(want, v["head.weight"], trans_b=True, bias=v["head.bias"])), t
            ops.greedy_tail(env.state, env.cfg(), y, v["head.weight"], v["head.bias"], t, env.obs, run.active, recs, run.nan_count,
                            noise=noise[t])
            run.active.fill_(1)                               # keep every env stepping: 40 steps of state for all of them
        assert differs_from_stateless == CAP - 1
        acts = recs["act"][recs["act"] >= 0]
        assert len(torch.unique(acts)) >= 3, torch.bincount(acts)


def _stateless_probs(pol):
    """policy_probs of `pol` evaluated from zero state at EVERY step: the control a route that drops its state would equal"""
    def probs(obs):
        z = pol.zero_state(obs.shape[0])
        return pol.step(obs.contiguous(), z[0], z[1])[:, :5]
    return probs


@pytest.mark.parametrize("name", list(POLICIES))
def test_tail_route_equals_the_stepwise_loop_at_every_chunk_size(ev, name):
    from uavppo import ops
    from uavppo.greedy import GreedyRun
    pol, fresh_env, noise, mode = _route_case(name)
    with ops.lstm_arith(mode):
        env = fresh_env()
        env.reset()
        acts = GreedyRun("lstm", pol, env, tail=True).chunk(0, CAP, noise)["act"]
        assert len(torch.unique(acts[acts >= 0])) >= 3, torch.bincount(acts[acts >= 0])        # the greedy actions vary ...
        with ops.lstm_arith("bf16x6") if name == "128x1_out_of_range" else ops.lstm_arith(mode):
            stateless = ev.evaluate(_stateless_probs(pol), fresh_env(), noise=noise, max_steps=CAP)
        assert ev.fused_refusal(pol, fresh_env()) is not None and ev.tail_refusal(pol, fresh_env()) is None
        want = ev.evaluate(pol, fresh_env(), noise=noise, max_steps=CAP, fused=False, tail=False)
        assert (want["steps"] < CAP).any(), want["steps"]                     # episodes end inside the cap
        assert not np.array_equal(want["steps"], stateless["steps"])          # ... and depend on the recurrent state
        for chunk in (1, 7, 40):
            _equal(ev.evaluate(pol, fresh_env(), noise=noise, max_steps=CAP, tail=True, chunk=chunk), want)
        _equal(ev.evaluate(pol, fresh_env(), noise=noise, max_steps=CAP), want)         # the default takes the tail route
    assert ops.get_lstm_arith() == "fp16x3"


def _threshold_controller(ev, N):
    pred = ev.ConcentrationThresholdPredictor(hidden_size=64, device=DEV, seed=4)
    pred.fc["fc.4.bias"].fill_(5.0)                       # thresholds inside the concentration range these short episodes see
    pred.fc["fc.4.weight"].mul_(6.0)
    return ev.ThresholdController(pred, (0.0, 100.0), N, device=DEV)


def _peak_stop(ev):
    pred = ev.PeakAndStopPredictor(device=DEV, seed=10)
    pred.heads_w[1].mul_(12.0)                            # a decisive stop head ...
    pred.lstm.p["weight_ih_l0"].mul_(250.0)               # ... on an LSTM that responds to concentrations / 100 of a few hundredths
    return pred


RULES = {
    "threshold_host": dict(thr=True, threshold_device=False),
    "threshold_device": dict(thr=True, threshold_device=True),
    "peak_host": dict(peak=True, peak_stop_device=False),
    "peak_device": dict(peak=True, peak_stop_device=True),
    "both_device": dict(thr=True, peak=True, threshold_device=True, peak_stop_device=True),
    "both_host": dict(thr=True, peak=True),
}


# every rule on the 64x2 policy (per-call layers); the C5 policy (steppers) takes both device rules at once
@pytest.mark.parametrize("name,rule", [("64x2", r) for r in RULES] + [("256x2_trend2", "both_device")])
def test_tail_route_equals_the_stepwise_loop_under_the_stop_rules(ev, name, rule):
    pol, fresh_env, noise, _ = _route_case(name)
    kw = dict(RULES[rule])
    thr, peak = kw.pop("thr", False), kw.pop("peak", False)
    outs = []
    for route in (dict(fused=False, tail=False), dict(tail=True), dict(tail=True, chunk=7)):
        ctl = _threshold_controller(ev, N_R) if thr else None
        outs.append(ev.evaluate(pol, fresh_env(), ctl, _peak_stop(ev) if peak else None, window_size_v21=12, noise=noise,
                                max_steps=CAP, **kw, **route))
    print(name, rule, "stopped early:", int(outs[0]["stopped_early"].sum()), "steps", outs[0]["steps"])
    assert outs[0]["stopped_early"].any() and not outs[0]["stopped_early"].all()          # the rules end some episodes, not all
    _equal(outs[1], outs[0])
    _equal(outs[2], outs[0])


@pytest.mark.parametrize("name", ["256x1", "64x2"])
def test_model_evaluator_writes_the_same_csv_on_the_tail_route(em, tmp_path, name):
    kw = dict(POLICIES[name])
    pol = _lstm_policy(kw.pop("H"), **kw)
    noise = torch.from_numpy(np.random.RandomState(9).randn(CAP, N_R, 2)).to(DEV)
    rows = {}
    for tag, route in (("stepwise", dict(fused=False, tail=False)), ("tail", dict(tail=True, chunk=7)), ("default", {})):
        evl = em.ModelEvaluator(pol, eval_episodes=N_R, device=DEV, env=_bank_env(N_R, "v1.1", 35, radius=200.0))
        out = evl.run_evaluation(noise=noise, max_steps=CAP, csv_path=str(tmp_path / f"{tag}.csv"), **route)
        rows[tag] = ((tmp_path / f"{tag}.csv").read_text(), out)
    assert (rows["stepwise"][1]["steps"] < CAP).any()
    for tag in ("tail", "default"):
        assert rows[tag][0] == rows["stepwise"][0]
        assert np.array_equal(rows[tag][1]["stopped_early"], rows["stepwise"][1]["stopped_early"])


def test_generate_expert_data_gives_the_same_pairs_on_the_tail_route():
    if PKG not in sys.path:
        sys.path.insert(0, PKG)
    import generate_expert_data as ged
    pol = _lstm_policy(256, seed=4, layers=2, obs_dim=8)
    want = ged.generate_expert_data(pol, num_episodes=N_R, variant="v2.1", seed=5, max_steps=CAP, out=None, fused=False, tail=False)
    for route in (dict(tail=True), {}):
        got = ged.generate_expert_data(pol, num_episodes=N_R, variant="v2.1", seed=5, max_steps=CAP, out=None, **route)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert want[0].shape == (len(want[1]), 8) and len(want[1]) >= N_R and len(np.unique(want[1])) >= 3


# ---------------------------------------------------------------------------------------------- 5. selection and refusals
def test_selection_and_refusals(ev, monkeypatch):
    from uavppo import ops
    from uavppo.policy import MLPActorCritic
    calls = []
    tail = ops.greedy_tail
    monkeypatch.setattr(ops, "greedy_tail", lambda *a, **k: (calls.append(1), tail(*a, **k))[1])
    env = _bank_env(N_R, "v2.0", 17)
    small_mlp = MLPActorCritic(6, 5, h1=128, h2=64, device=DEV, seed=1)
    with pytest.raises(RuntimeError, match=r"evaluate\(tail=True\): MLP 6-128-64-5"):
        ev.evaluate(small_mlp, env, max_steps=4, tail=True)
    with pytest.raises(RuntimeError, match=r"evaluate\(tail=True\): the policy's obs_dim is 7"):
        ev.evaluate(_lstm_policy(256, seed=1, obs_dim=7), env, max_steps=4, tail=True)
    with pytest.raises(RuntimeError, match=r"evaluate\(tail=True\): a policy_probs function has no tail route"):
        ev.evaluate(lambda o: o[:, :5], env, max_steps=4, tail=True)
    h256 = _lstm_policy(256, seed=1)
    with pytest.raises(RuntimeError, match=r"evaluate\(fused=True\): LSTM 1 layer\(s\), hidden 256"):
        ev.evaluate(h256, env, max_steps=4, fused=True)
    with pytest.raises(RuntimeError, match=r"evaluate\(fused=True\): LSTM 1 layer\(s\), hidden 256"):
        ev.evaluate(h256, env, max_steps=4, fused=True, tail=True)
    # the refusals say what the default route then does
    for pol, fused_ok, tail_ok in ((h256, False, True), (small_mlp, False, False), (_lstm_policy(64, seed=1), True, True)):
        assert (ev.fused_refusal(pol, env) is None) == fused_ok and (ev.tail_refusal(pol, env) is None) == tail_ok
        del calls[:]
        ev.evaluate(pol, env, max_steps=4)
        assert bool(calls) == (tail_ok and not fused_ok)
        del calls[:]
        ev.evaluate(pol, env, max_steps=4, tail=False)
        assert not calls
    del calls[:]
    ev.evaluate(h256, env, max_steps=4, fused=False)                        # fused=False alone still means the step-wise loop
    assert not calls
    ev.evaluate(_lstm_policy(64, seed=1), env, max_steps=4, tail=True)      # the tail route covers what the fused kernel covers too
    assert len(calls) == 4
