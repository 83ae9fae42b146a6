"""ModelEvaluator (evaluate_model.py) and the entry points behind it -- uav_greedy_episodes_stop (the fused greedy-episode
kernels with the stop rule of PPOV1.1/evaluate_model.py:25-37 on the device) and uav_stop_stability (the step-wise path) --
against CPU oracle episodes (tests/_eval_v11_check.py over OracleVecEnv: f64 policy, the restated f32 rule pinned by
tests/test_eval_v11_rule.py), themselves under chunking, and uav_greedy_episodes under a rule that cannot fire.  -m gpu.

Tolerances: positions / deviations 2e-3 and the top-2 logit GAP of tests/test_gpu_greedy_eval.py; rule_val exact where the
window's positions are bit-equal to the oracle's and 4e-3 otherwise (a position error d per sample moves a std by at most
2 d).  On the step-wise path there are no position or flag records, so rule_val is only held to 4e-3 there; that
uav_stop_stability computes the restated rule bit for bit is test_stop_stability_equals_the_restated_rule_bit_for_bit's.

Decisions are compared for EVERY env, which the margins asserted on the oracle make meaningful:
  * |pos_std - 2.0| >= 1e-2 at every step: 2.5 times what the position tolerance can move a std;
  * the concentration chain at least CONC_MARGIN = 1e-6 (in units of obs[2]) away from its threshold.  1e-6 is the loosest
    tolerance tests/test_gpu_env.py gives a concentration-derived quantity (obs itself is compared exactly there), and it
    is enough only because the comparison here holds the device to it as well: obs[2] of every stepped step, on the fused
    and the step-wise path, is asserted to lie within CONC_MARGIN of the oracle's (_compare_obs2).  A position that drifted
    by the 2e-3 px the position comparison allows, in a cell where the field is steep enough to move the sampled
    concentration by more than that, fails there by name; no bound on the field's gradient is needed, and a device
    concentration within CONC_MARGIN of an oracle value that is more than CONC_MARGIN from the threshold lies on the
    oracle's side of it."""
import os
import sys

import numpy as np
import pytest
import torch

import _eval_v11_check as ck
from oracle import ppo_oracle as po
from oracle.env_oracle import FieldBank

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "uav-wrf-les-ppo-lstm_amd")
GAP = 1e-4                    # as tests/test_gpu_greedy_eval.py
POS_TOL = 2e-3
STD_MARGIN, CONC_MARGIN = 1e-2, 1e-6
TOWARDS = [0.0, 2.0, -5.0, 2.0, -5.0]    # head bias: +x / +y from the corner

# kind, policy seed, head bias, bank seed, N, cap.  Seeds fixed after checking margins and coverage with the oracle alone.
CASES = {
    "mlp": ("mlp", 3, TOWARDS, 31, 24, 120),
    "mlp_free": ("mlp", 3, None, 32, 24, 120),
    "lstm64": ("lstm64", 6, TOWARDS, 33, 24, 120),
    "lstm128": ("lstm128", 5, None, 34, 24, 120),
    "stepwise_2x64": ("lstm64x2", 3, TOWARDS, 35, 16, 100),
    "stepwise_mlp": ("mlp", 3, TOWARDS, 31, 24, 120),
}


@pytest.fixture(scope="module")
def em():
    if PKG not in sys.path:
        sys.path.insert(0, PKG)
    import evaluate_model as m
    return m


def make_policy(kind, seed, bias, device):
    from uavppo.policy import LSTMActorCritic, MLPActorCritic
    if kind == "mlp":
        pol = MLPActorCritic(6, 5, device=device, seed=seed)
        pol.views["head.weight"][:5].mul_(40.0)           # a decisive greedy policy (actor rows of gain 0.01 otherwise)
    else:
        H, _, layers = kind[4:].partition("x")
        pol = LSTMActorCritic(6, int(H), int(layers or 1), device=device, seed=seed)
        pol.views["head.weight"][:5].mul_(400.0)
    if bias is not None:
        pol.views["head.bias"][:5].copy_(torch.tensor(bias))
    return pol


def oracle_logits(kind, pol):
    """() -> per-episode f64 logits function of the policy's parameters (LSTM state from zero)."""
    p = {k: v.detach().cpu().double() for k, v in pol.named_views().items()}
    if kind == "mlp":
        def fresh():
            def f(obs):
                with torch.no_grad():
                    return po.mlp_forward(p, torch.from_numpy(obs.astype(np.float64))[None])[2][0].numpy()
            return f
        return fresh
    L, H = pol.num_layers, pol.hidden

    def fresh():
        st = [torch.zeros(L, 1, H, dtype=torch.float64), torch.zeros(L, 1, H, dtype=torch.float64)]

        def f(obs):
            with torch.no_grad():
                _, _, logits, (st[0], st[1]) = po.lstm_policy_forward(p, torch.from_numpy(obs.astype(np.float64))[None, None], st[0], st[1])
            return logits[0, 0].numpy()
        return f
    return fresh


_ORACLE = {}


def case_oracle(name):
    """(bank, noise, oracle results) of a case; the oracle's policy is the CPU twin of the device policy (same seed, same
    f32 parameters)."""
    if name not in _ORACLE:
        kind, seed, bias, bseed, N, cap = CASES[name]
        pol = make_policy(kind, seed, bias, "cpu")
        bank = FieldBank.from_seed(N, "v1.1", seed=bseed)
        noise = np.random.RandomState(1000 + bseed).randn(cap, N, 2)
        _ORACLE[name] = (bank, noise, ck.oracle_episodes(oracle_logits(kind, pol), bank, N, cap, noise))
    return _ORACLE[name]


def _env(bank, N):
    from uavppo.vec_env import VecMethaneEnv
    return VecMethaneEnv(N, "v1.1", DEV, seed=3, bank=bank.interleaved(), bank_sources=bank.sources)


def _assert_margins(want):
    assert want["gap"] > GAP, f"oracle's smallest top-2 logit gap {want['gap']:g}: agreement would be luck"
    assert want["std_margin"] >= STD_MARGIN, want["std_margin"]
    assert want["conc_margin"] > CONC_MARGIN, want["conc_margin"]


def _compare_rule_val(got_val, got_pos, want, steps, window=ck.WINDOW):
    """rule_val [N][T] against the oracle's: NaN pattern equal; the value exact where the whole window's positions are
    bit-equal, within 4e-3 otherwise."""
    n_exact = 0
    for i in range(len(steps)):
        for t in range(int(steps[i])):
            w, g = want["rule_val"][i, t], got_val[i, t]
            assert np.isnan(w) == np.isnan(g), (i, t)
            if np.isnan(w):
                continue
            same = np.array_equal(got_pos[i, t + 1 - window:t + 1].view(np.uint32), want["pos_rec"][i, t + 1 - window:t + 1].view(np.uint32))
            if same:
                assert g.view(np.uint32) == w.view(np.uint32), (i, t, float(g), float(w))
                n_exact += 1
            else:
                assert abs(float(g) - float(w)) <= 4e-3, (i, t, float(g), float(w))
        assert np.isnan(got_val[i, int(steps[i]):]).all(), i
    return n_exact


def _compare_obs2(got, want, steps):
    """obs[2] each stepped step returned, [N][T], within CONC_MARGIN of the oracle's (see the module docstring)."""
    for i in range(len(steps)):
        k = int(steps[i])
        err = np.abs(got[i, :k].astype(np.float64) - want["obs2_rec"][i, :k].astype(np.float64))
        assert (err <= CONC_MARGIN).all(), (i, int(err.argmax()), float(err.max()))


def _compare(out, rec, want, stepwise=False):
    steps = want["steps"]
    assert np.array_equal(out["steps"], steps), (out["steps"], steps)
    assert np.array_equal(out["stopped_early"], want["stopped"])
    assert np.array_equal(out["success"], want["success"])
    assert np.allclose(out["deviations"], want["deviations"], rtol=0, atol=POS_TOL)
    assert np.allclose(out["final_conc"], want["final_conc"], rtol=0, atol=2 * 100 * CONC_MARGIN)
    assert out["final_conc"].dtype == np.float32
    val = rec["rule_val"].cpu().numpy()
    if stepwise:
        _compare_obs2(rec["obs2"].cpu().numpy(), want, steps)
        # no records on this path; rule_val [N][steps run]: compare the decision-bearing values while the env was active
        for i in range(len(steps)):
            for t in range(int(steps[i])):
                w, g = want["rule_val"][i, t], val[i, t]
                assert np.isnan(w) == np.isnan(g), (i, t)
                assert np.isnan(w) or abs(float(g) - float(w)) <= 4e-3, (i, t, float(g), float(w))
        return 0
    flags = rec["flags"].cpu().numpy()
    T = flags.shape[1]
    assert np.array_equal(flags & 8, want["flags"][:, :T] & 8)                    # bit3 of every record of every env
    assert np.array_equal(flags, want["flags"][:, :T])                           # and done / reached / not stepped
    _compare_obs2(rec["obs"].cpu().numpy()[:, :, 2], want, steps)
    pos = rec["pos"].cpu().numpy()
    for i in range(len(steps)):
        assert np.allclose(pos[i, :steps[i]], want["pos_rec"][i, :steps[i]], rtol=0, atol=POS_TOL)
    return _compare_rule_val(val, pos, want, steps)


# ---------------------------------------------------------------------------------------------- 1. against the oracle
def _run_case(em, name, fused):
    bank, noise, want = case_oracle(name)
    _assert_margins(want)
    kind, seed, bias, _, N, cap = CASES[name]
    pol = make_policy(kind, seed, bias, DEV)
    evl = em.ModelEvaluator(pol, eval_episodes=N, device=DEV, env=_env(bank, N))
    assert (evl.position_window, evl.stability_threshold, evl.conc_threshold, evl.eval_episodes) == (10, 2.0, 80.0, N)
    nz = torch.from_numpy(noise).to(DEV)
    # the public call ...
    out = evl.run_evaluation(noise=nz, max_steps=cap, fused=fused, csv_path=None)
    # ... and the same episodes with the records kept, for the per-step comparison
    evl.env.reset()
    kind, core = em._policy_core_checked(pol)
    rec = {}
    if fused:
        res = evl._episodes_fused(kind, core, nz, cap, 50, want=rec)
    else:
        res = evl._episodes_stepwise(kind, core, nz, cap, want=rec)
    assert np.array_equal(res[0].cpu().numpy(), out["steps"]) and np.array_equal(res[3].cpu().numpy(), out["stopped_early"])
    n_exact = _compare(out, rec, want, stepwise=not fused)
    return want, n_exact


@pytest.mark.parametrize("name", ["mlp", "mlp_free", "lstm64", "lstm128"])
def test_fused_matches_oracle(em, name):
    want, n_exact = _run_case(em, name, fused=True)
    assert n_exact > 0, "no window with bit-equal positions: the exact comparison of rule_val went untested"


@pytest.mark.parametrize("name", ["stepwise_2x64", "stepwise_mlp"])
def test_stepwise_matches_oracle(em, name):
    if name == "stepwise_2x64":          # a policy the fused kernels refuse takes the step-wise path by itself
        from uavppo.vec_env import VecMethaneEnv
        evl = em.ModelEvaluator(make_policy(*CASES[name][:3], DEV), eval_episodes=4, device=DEV, env=VecMethaneEnv(4, "v1.1", DEV))
        with pytest.raises(RuntimeError, match="2 layer"):
            evl.run_evaluation(max_steps=5, fused=True, csv_path=None)
        assert evl.run_evaluation(max_steps=12, csv_path=None)["steps"].shape == (4,)
    _run_case(em, name, fused=False)


def test_cases_cover_the_rule(em):
    """Asserted on the oracle's results: a step-10 stop, a later stop, a cap, and an episode ended by `reached`."""
    seen = {"stop10": False, "later": False, "cap": False, "reached": False, "stable_low_conc": False}
    for name in CASES:
        want = case_oracle(name)[2]
        cap = CASES[name][5]
        seen["stop10"] |= bool((want["stopped"] & (want["steps"] == 10)).any())
        seen["later"] |= bool((want["stopped"] & (want["steps"] > 10)).any())
        seen["cap"] |= bool((~want["stopped"] & ~want["reached"] & (want["steps"] == cap)).any())
        seen["reached"] |= bool((want["reached"] & ~want["stopped"]).any())
        stable = want["rule_val"] < np.float32(2.0)
        seen["stable_low_conc"] |= bool((stable & ((want["flags"] & 8) == 0) & ((want["flags"] & 4) == 0)).any())
    assert all(seen.values()), seen


# ---------------------------------------------------------------------------------------------- 2. chunking, frozen state
def _raw_run(pol, bank, N, cap, noise, chunks, rule, H, frozen=None, with_val=True):
    """uav_greedy_episodes_stop in `chunks` steps per call; returns everything that must not depend on the chunking."""
    from uavppo import ops
    env = _env(bank, N)
    env.reset()
    cur = env.obs
    g = torch.Generator().manual_seed(0)
    h = (torch.rand(N, H, generator=g) * 0.2).to(DEV) if H else None
    c = (torch.rand(N, H, generator=g) * 0.2).to(DEV) if H else None
    active = torch.ones(N, dtype=torch.uint8, device=DEV) if frozen is None else (~frozen).to(torch.uint8)
    win = torch.zeros(N, rule.window, 2, device=DEV)
    cnt = torch.zeros(N, dtype=torch.int32, device=DEV)
    nan = torch.zeros(1, dtype=torch.int32, device=DEV)
    recs = {"act": [], "obs": [], "pos": [], "flags": [], "val": []}
    snaps = []
    t0 = 0
    for k in chunks:
        r = {"act": torch.empty(N, k, dtype=torch.int32, device=DEV), "obs": torch.empty(N, k, 6, device=DEV),
             "pos": torch.empty(N, k, 2, device=DEV), "flags": torch.empty(N, k, dtype=torch.uint8, device=DEV)}
        val = torch.empty(N, k, device=DEV) if with_val else None
        ops.greedy_episodes_stop(env.state, N, env.cfg(), pol.flat, H, k, cur, h, c, active, r, rule, win, cnt,
                                 noise=noise[:, t0:t0 + k].contiguous(), nan_count=nan, rule_val=val)
        for key in ("act", "obs", "pos", "flags"):
            recs[key].append(r[key])
        recs["val"].append(val if with_val else torch.zeros(N, k, device=DEV))
        snaps.append((t0 + k, env.state.clone(), cur.clone(), None if h is None else h.clone(), None if c is None else c.clone(),
                      win.clone(), cnt.clone(), active.clone()))
        t0 += k
    recs = {key: torch.cat(v, 1).cpu() for key, v in recs.items()}
    final = [env.state.cpu(), cur.cpu(), None if h is None else h.cpu(), None if c is None else c.cpu(), win.cpu(), cnt.cpu(),
             active.cpu(), int(nan.item())]
    return recs, final, snaps


def _same(a, b):
    if a is None or b is None:
        return a is None and b is None
    if torch.is_tensor(a):
        return torch.equal(a.view(torch.uint8) if a.dtype != torch.uint8 else a, b.view(torch.uint8) if b.dtype != torch.uint8 else b)
    return a == b


@pytest.mark.parametrize("name", ["mlp", "lstm64", "lstm128"])
def test_chunking_is_invisible_and_stopped_envs_stay_frozen(em, name):
    from uavppo import ops
    kind, seed, bias, bseed, N, cap = CASES[name]
    pol = make_policy(kind, seed, bias, DEV)
    H = pol.hidden if kind != "mlp" else 0
    bank = FieldBank.from_seed(N, "v1.1", seed=bseed)
    noise = torch.from_numpy(np.random.RandomState(1000 + bseed).randn(cap, N, 2)).to(DEV).transpose(0, 1).contiguous()
    rule = ops.make_stop_rule()
    frozen = torch.arange(N, device=DEV) % 5 == 3                    # these come in inactive
    runs = {}
    for label, chunks in (("one", [cap]), ("7", [7] * (cap // 7) + ([cap % 7] if cap % 7 else [])), ("1", [1] * cap),
                          ("13+", [13, 4, 3, cap - 20])):              # 7, 13, 4, 3, 1: all cut a 10-step window in two
        assert sum(chunks) == cap
        runs[label] = _raw_run(pol, bank, N, cap, noise, chunks, rule, H, frozen)
    ref = runs["one"]
    for label, r in runs.items():
        for key in ref[0]:
            assert _same(ref[0][key], r[0][key]), (label, key)            # records and rule_val, NaN patterns included
        for i, (a, b) in enumerate(zip(ref[1], r[1])):
            assert _same(a, b), (label, i)                                # blob, cur_obs, h, c, stop_win, stop_cnt, active, nan
    flags = ref[0]["flags"]
    assert ref[1][7] == 0
    assert (flags[frozen.cpu()] == 4).all() and (ref[1][5][frozen.cpu()] == 0).all()         # never stepped: no window either
    # rule_val = NULL changes nothing but the missing output
    lean = _raw_run(pol, bank, N, cap, noise, [7] * (cap // 7) + ([cap % 7] if cap % 7 else []), rule, H, frozen, with_val=False)
    for key in ("act", "obs", "pos", "flags"):
        assert _same(ref[0][key], lean[0][key]), key
    for i, (a, b) in enumerate(zip(ref[1], lean[1])):
        assert _same(a, b), i
    # frozen state: in the run of single steps, an env the rule stopped at step s has the blob, observation, h, c, window
    # and count that step s left, at every later snapshot; its later records say "not stepped"
    snaps = runs["1"][2]
    hit = (flags & 8) != 0
    assert hit.any(), "the rule stopped no env: freezing went untested"
    assert (hit.sum(1) <= 1).all()
    n_checked = 0
    for n in torch.nonzero(hit.any(1)).reshape(-1).tolist():
        s = int(hit[n].int().argmax())                                    # record index of the stopping step
        assert (flags[n, s + 1:] == 4).all() and (flags[n, :s + 1] & 4 == 0).all()
        assert int(snaps[s][7][n]) == 0 and (s == 0 or int(snaps[s - 1][7][n]) == 1)
        for later in (s + 1, cap - 1):
            if later >= cap or later == s:
                continue
            for idx in (2, 3, 4, 5, 6):                                   # cur_obs, h, c, stop_win, stop_cnt
                a, b = snaps[s][idx], snaps[later][idx]
                assert (a is None and b is None) or torch.equal(a[n], b[n]), (n, idx)
            n_checked += 1
    # the state blob is struct-of-arrays: compare the peek view of stopped envs between the stopping step and the end
    env_a, env_b = _env(bank, N), _env(bank, N)
    stopped_envs = torch.nonzero(hit.any(1)).reshape(-1)
    first = int(hit.int().argmax(1)[stopped_envs].max())                  # after this record every stopped env is frozen
    if first + 1 < cap:
        env_a.state.copy_(snaps[first][1])
        env_b.state.copy_(snaps[cap - 1][1])
        for a, b in zip(env_a.peek(), env_b.peek()):
            assert torch.equal(a[stopped_envs.to(DEV)], b[stopped_envs.to(DEV)])
    assert n_checked > 0


# ---------------------------------------------------------------------------------------------- 3. neutral rule, refusals
@pytest.mark.parametrize("name", ["mlp", "lstm64", "lstm128"])
def test_a_rule_that_cannot_fire_gives_uav_greedy_episodes(em, name):
    from uavppo import ops
    kind, seed, bias, bseed, N, cap = CASES[name]
    pol = make_policy(kind, seed, bias, DEV)
    H = pol.hidden if kind != "mlp" else 0
    bank = FieldBank.from_seed(N, "v1.1", seed=bseed)
    noise = torch.from_numpy(np.random.RandomState(1000 + bseed).randn(cap, N, 2)).to(DEV).transpose(0, 1).contiguous()
    never = ops.make_stop_rule(pos_std_max=0.0)
    recs, final, _ = _raw_run(pol, bank, N, cap, noise, [cap], never, H)
    assert ((recs["flags"] & 8) == 0).all()
    # the same through uav_greedy_episodes
    env = _env(bank, N)
    env.reset()
    g = torch.Generator().manual_seed(0)
    h = (torch.rand(N, H, generator=g) * 0.2).to(DEV) if H else None
    c = (torch.rand(N, H, generator=g) * 0.2).to(DEV) if H else None
    active = torch.ones(N, dtype=torch.uint8, device=DEV)
    nan = torch.zeros(1, dtype=torch.int32, device=DEV)
    r = {"act": torch.empty(N, cap, dtype=torch.int32, device=DEV), "obs": torch.empty(N, cap, 6, device=DEV),
         "pos": torch.empty(N, cap, 2, device=DEV), "flags": torch.empty(N, cap, dtype=torch.uint8, device=DEV)}
    ops.greedy_episodes(env.state, N, env.cfg(), pol.flat, H, cap, env.obs, h, c, active, r, noise=noise, nan_count=nan)
    for key in ("act", "obs", "pos", "flags"):
        assert _same(recs[key], r[key].cpu()), key
    for a, b in zip(final[:4] + [final[6]], [env.state.cpu(), env.obs.cpu(), None if h is None else h.cpu(),
                                             None if c is None else c.cpu(), active.cpu()]):
        assert _same(a, b)
    # the window it kept is the last positions of the records, oldest first
    flags, pos = recs["flags"], recs["pos"]
    for n in range(N):
        stepped = torch.nonzero((flags[n] & 4) == 0).reshape(-1)
        k = min(len(stepped), never.window)
        assert int(final[5][n]) == k
        assert torch.equal(final[4][n, :k], pos[n, stepped[len(stepped) - k:]])


def test_refusals_name_their_reason(em):
    from uavppo import ops
    from uavppo._lib import StopRule
    N = 16
    bank = FieldBank.from_seed(N, "v1.1", seed=5)
    env = _env(bank, N)
    env.reset()
    pol = make_policy("mlp", 1, None, DEV)
    recs = {"act": torch.empty(N, 4, dtype=torch.int32, device=DEV), "obs": torch.empty(N, 4, 6, device=DEV),
            "pos": torch.empty(N, 4, 2, device=DEV), "flags": torch.full((N, 4), 0xA5, dtype=torch.uint8, device=DEV)}
    act = torch.ones(N, dtype=torch.uint8, device=DEV)
    cnt = torch.zeros(N, dtype=torch.int32, device=DEV)
    wide = StopRule(17, 2.0, 2.0, 100.0, 80.0)
    with pytest.raises(RuntimeError, match=r"uav_greedy_episodes_stop.*window=17"):
        ops.greedy_episodes_stop(env.state, N, env.cfg(), pol.flat, 0, 4, env.obs, None, None, act, recs, wide,
                                 torch.zeros(N, 17, 2, device=DEV), cnt)
    with pytest.raises(RuntimeError, match=r"uav_greedy_episodes_stop.*NULL stop_win"):
        ops.greedy_episodes_stop(env.state, N, env.cfg(), pol.flat, 0, 4, env.obs, None, None, act, recs, ops.make_stop_rule(),
                                 None, cnt)
    with pytest.raises(RuntimeError, match=r"uav_stop_stability.*window=17"):
        ops.stop_stability(wide, torch.zeros(N, 2, device=DEV), torch.zeros(N, device=DEV), torch.zeros(N, 17, 2, device=DEV), cnt)
    with pytest.raises(RuntimeError, match=r"uav_stop_stability.*NULL stop_win"):
        ops.stop_stability(ops.make_stop_rule(), torch.zeros(N, 2, device=DEV), torch.zeros(N, device=DEV), None, cnt)
    with pytest.raises(RuntimeError, match="window 17 outside"):
        ops.make_stop_rule(window=17)
    assert (recs["flags"].cpu() == 0xA5).all() and int(cnt.sum()) == 0     # nothing ran: no record written, no window filled


# ---------------------------------------------------------------------------------------------- 4. uav_stop_stability alone
def test_stop_stability_equals_the_restated_rule_bit_for_bit():
    """Random windows (a third of them within 1e-3 of the threshold), fed step by step: value bits and decisions equal the
    numpy restatement's; inactive envs keep their window."""
    from uavppo import ops
    rng = np.random.default_rng(1)
    N, T = 600, 14
    base = rng.random((N, 1, 2)) * 480 + 10
    walk = rng.standard_normal((N, T, 2)) * rng.uniform(0.3, 4.0, (N, 1, 1))
    third = np.arange(N) % 3 == 0
    sd = np.std(walk[:, -10:], axis=1).mean(1)
    walk[third] *= ((2.0 + rng.uniform(-9e-4, 9e-4, N)) / sd)[third, None, None]
    pos = (base + walk).astype(np.float32)
    obs2 = (rng.random((N, T)) * 0.01).astype(np.float32)               # around the concentration threshold (0.004)
    sleepy = np.arange(N) % 7 == 2                                       # inactive at step 11 only
    rule = ops.make_stop_rule()
    win = torch.zeros(N, 10, 2, device=DEV)
    cnt = torch.zeros(N, dtype=torch.int32, device=DEV)
    hist = [[] for _ in range(N)]
    near = 0
    for t in range(T):
        act = np.ones(N, np.uint8)
        if t == 11:
            act[sleepy] = 0
        o2 = torch.from_numpy(np.ascontiguousarray(np.stack([obs2[:, t]] * 3, 1))).to(DEV)[:, 1]      # a strided column view
        stop, val = ops.stop_stability(rule, torch.from_numpy(pos[:, t].copy()).to(DEV), o2, win, cnt,
                                       active=torch.from_numpy(act).to(DEV))
        stop, val = stop.cpu().numpy(), val.cpu().numpy()
        for n in range(N):
            if not act[n]:
                assert stop[n] == 0 and np.isnan(val[n])
                continue
            hist[n].append(pos[n, t])
            w_stop, w_val = ck.rule(hist[n], obs2[n, t])
            assert np.isnan(w_val) == np.isnan(val[n]), (n, t)
            if not np.isnan(w_val):
                assert val[n].view(np.uint32) == np.float32(w_val).view(np.uint32), (n, t, float(val[n]), float(w_val))
                near += abs(float(w_val) - 2.0) < 1e-3
            assert bool(stop[n]) == w_stop, (n, t)
    assert near >= 100, near
    got_win, got_cnt = win.cpu().numpy(), cnt.cpu().numpy()
    for n in range(N):
        assert got_cnt[n] == 10 and np.array_equal(got_win[n], np.asarray(hist[n][-10:], np.float32))


# ---------------------------------------------------------------------------------------------- 5. the public surface
def test_model_path_csv_and_main(em, tmp_path, monkeypatch):
    """A reference-keyed .pth goes through _load_model into PPOActorCritic(6, 5); the CSV holds the returned arrays in the
    reference's columns; the policy object of the same parameters gives the same evaluation bit for bit; main() runs."""
    from uavppo.policy import MLPActorCritic
    from uavppo.vec_env import VecMethaneEnv
    core = make_policy("mlp", 3, TOWARDS, "cpu")
    assert sorted(core.state_dict()) == sorted(MLPActorCritic.KEYS)
    (tmp_path / "model").mkdir()
    path = tmp_path / "model" / "ppo_successful_models.pth"
    torch.save(core.state_dict(), str(path))
    N = 32
    evl = em.ModelEvaluator(str(path), eval_episodes=N, device=DEV)
    assert type(evl.model).__name__ == "PPOActorCritic" and evl.env.variant == "v1.1" and evl.env.current_radius == 50.0
    assert torch.equal(evl.model.core.flat.cpu(), core.flat)
    csv = tmp_path / "out.csv"
    out = evl.run_evaluation(max_steps=80, csv_path=str(csv))
    assert sorted(out) == ["deviations", "final_conc", "steps", "stopped_early", "success"]
    lines = csv.read_text().splitlines()
    assert lines[0] == "episode,steps,deviation,success,final_conc" and len(lines) == N + 1
    for i, ln in enumerate(lines[1:]):
        ep, st, dv, ok, fc = ln.split(",")
        assert (int(ep), int(st), float(dv), ok, np.float32(fc)) == (i + 1, out["steps"][i], out["deviations"][i],
                                                                      str(bool(out["success"][i])), out["final_conc"][i])
    assert (out["steps"] >= 1).all() and (out["steps"] <= 80).all()
    assert np.array_equal(out["success"], out["deviations"] < 50.0)
    for kw in ({"fused": True}, {"fused": False}):
        other = em.ModelEvaluator(make_policy("mlp", 3, TOWARDS, DEV), eval_episodes=N, device=DEV,
                                  env=VecMethaneEnv(N, "v1.1", DEV)).run_evaluation(max_steps=80, csv_path=None, **kw)
        for k in ("steps", "stopped_early", "success"):
            assert np.array_equal(out[k], other[k]), (kw, k)
        if kw["fused"]:
            assert np.array_equal(out["deviations"], other["deviations"]) and np.array_equal(out["final_conc"], other["final_conc"])
    with pytest.raises(ValueError, match="eval_episodes"):
        em.ModelEvaluator(core, eval_episodes=5, device=DEV, env=VecMethaneEnv(4, "v1.1", DEV))
    with pytest.raises(TypeError, match="expected a model path"):
        em.ModelEvaluator(lambda o: o, eval_episodes=4, device=DEV)
    monkeypatch.chdir(tmp_path)
    m = em.main(num_envs=16, device=DEV)
    assert m is not None and m["steps"].shape == (16,) and os.path.exists(tmp_path / "evaluation_results.csv")
    assert em.main(num_envs=4, model_path="model/none.pth", device=DEV) is None


@pytest.mark.parametrize("kind", ["mlp", "lstm64"])
@pytest.mark.parametrize("fused", [True, False])
def test_nan_parameters_raise(em, kind, fused):
    from uavppo.vec_env import VecMethaneEnv
    pol = make_policy(kind, 1, None, DEV)
    pol.flat[3] = float("nan")
    evl = em.ModelEvaluator(pol, eval_episodes=16, device=DEV, env=VecMethaneEnv(16, "v1.1", DEV))
    with pytest.raises(RuntimeError, match="NaN in probs"):
        evl.run_evaluation(max_steps=20, fused=fused, csv_path=None)
