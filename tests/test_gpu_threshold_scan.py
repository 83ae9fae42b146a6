"""uav_threshold_windows / uav_threshold_rule (csrc/threshold.hip: the PPOV2.0 ThresholdController's rule over a chunk of records,
around one batched call of the ConcentrationThresholdPredictor) and evaluate(..., threshold_device=True) on top of them.  -m gpu.

The kernels are compared bit for bit with their numpy restatement (tests/_threshold_check.py, itself pinned to np.mean and to the
reference's recorded controller traces by tests/test_threshold_host.py).  Through the predictor, thresholds are compared with the
f32 CPU oracle (oracle.eval_oracle.ThresholdPredictorOracle) within TOL = 0.95 * (2e-4 + 2e-5 |pred|), the bound
tests/test_gpu_eval.py accepts for this predictor on the GPU, and decisions exactly -- which is sound because every scenario asserts
on the oracle's side that each |cur - thr| and |mean - thr| it meets while an episode is live exceeds MARGIN = 5 TOL at the
scenario's largest threshold."""
import os

import numpy as np
import pytest
import torch

from _threshold_check import FACTOR, REFERENCE, is_update, live_margin, rule_ref, slots, windows_ref
from oracle import eval_oracle as eo
from oracle import ppo_oracle as po
from oracle.env_oracle import FieldBank, OracleVecEnv
from test_gpu_greedy_eval import GAP, TOWARDS, _agree, _bank_env, _equal, _lstm_policy, _oracle_lstm, ev  # noqa: F401
from test_gpu_peak_stop import TOL as PEAK_TOL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = os.path.join(os.path.dirname(__file__), "golden", "eval_v20.npz")


def tol(pred):
    return FACTOR * (2e-4 + 2e-5 * abs(pred))


def margin_needed(thr_max):
    """5 TOL at the scenario's largest threshold (thr = 0.95 pred)"""
    return 5.0 * tol(thr_max / FACTOR)


@pytest.fixture(scope="module")
def ops():
    from uavppo import ops as o
    return o


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64, 1: np.uint8}[a.dtype.itemsize])


# ---------------------------------------------------------------------------------------------- kernel cases
PARAMS = {"ref": dict(window=10, every=10, min_steps=20), "w7e4m9": dict(window=7, every=4, min_steps=9)}
SCALER = (0.22199317, 100.64873914)          # lo, scale: the golden's MinMaxScaler
# (n, steps, step_cnt): plain; the single step is the first update step; no update step at all; slots differ per env, hist partly
# filled accordingly; plain
CASES = {"19x37": (19, 37, 0), "1x1_update": (1, 1, 19), "1x1_none": (1, 1, 18), "3x25_slots": (3, 25, [0, 7, 15]), "16x16": (16, 16, 0)}


def make_series(n, steps, seed):
    """concentrations / 100 as f32: each env its own level, so that the rule fires for some and not for others"""
    rng = np.random.RandomState(seed)
    level = rng.uniform(0.2, 1.0, (n, 1))
    return (rng.uniform(0.0, 1.0, (n, steps)) * level).astype(np.float32)


def case_inputs(case, p):
    n, steps, cnt = CASES[case]
    w = p["window"]
    series = make_series(n, steps, seed=100 * n + steps + w)
    rng = np.random.RandomState(n + w)
    hist = rng.uniform(0.0, 1.0, (n, w - 1)).astype(np.float32)          # beyond the fill: values nobody may read
    return series, hist, np.broadcast_to(np.asarray(cnt, np.int32), (n,)).copy()


def pred_table(n, seed, lo=35.0, hi=110.0):
    """a synthetic predictor: pred of env e's update step t is table[e, t // every]"""
    return np.random.RandomState(seed).uniform(lo, hi, (n, 64)).astype(np.float32)


def pred_for(table, cnt, steps, every):
    S = slots(steps, every)
    return np.stack([table[e, int(cnt[e]) // every + 1:int(cnt[e]) // every + 1 + S] for e in range(len(cnt))])


def gpu_windows(ops, series, hist, cnt, active=None, **kw):
    s = series if torch.is_tensor(series) else torch.from_numpy(series).to(DEV)
    h, c = torch.from_numpy(hist).to(DEV), torch.from_numpy(cnt).to(DEV)
    a = None if active is None else torch.from_numpy(np.asarray(active, np.uint8)).to(DEV)
    x = ops.threshold_windows(s, h, c, active=a, **kw)
    return x.cpu().numpy(), h.cpu().numpy(), c.cpu().numpy()


def gpu_rule(ops, series, hist, cnt, pred, thr, active=None, **kw):
    """-> first_hit, stop, thr_out, thr, hist, cnt as numpy (the order of rule_ref)"""
    s = series if torch.is_tensor(series) else torch.from_numpy(series).to(DEV)
    h, c = torch.from_numpy(hist).to(DEV), torch.from_numpy(cnt).to(DEV)
    p, th = torch.from_numpy(np.ascontiguousarray(pred)).to(DEV), torch.from_numpy(np.asarray(thr, np.float64)).to(DEV)
    a = None if active is None else torch.from_numpy(np.asarray(active, np.uint8)).to(DEV)
    first, stop, thr_out = ops.threshold_rule(s, h, c, p, th, active=a, **kw)
    return first.cpu().numpy(), stop.cpu().numpy(), thr_out.cpu().numpy(), th.cpu().numpy(), h.cpu().numpy(), c.cpu().numpy()


def _same(got, want, what):
    for name, a, b in zip(("first_hit", "stop", "thr_out", "thr", "hist", "step_cnt"), got, want):
        assert a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b)), (what, name, a, b)


# ---------------------------------------------------------------------------------------------- 1. windows
@pytest.mark.parametrize("pname", list(PARAMS))
def test_windows_are_the_restatement_bit_for_bit(ops, pname):
    p = PARAMS[pname]
    lo, scale = SCALER
    filled = 0
    for case in CASES:
        series, hist, cnt = case_inputs(case, p)
        n, steps = series.shape
        want = windows_ref(series, hist, cnt, lo=lo, scale=scale, **p)
        x, hist_g, cnt_g = gpu_windows(ops, series, hist, cnt, lo=lo, scale=scale, **p)
        assert x.shape == (n, slots(steps, p["every"]), p["window"]) and np.array_equal(_bits(x), _bits(want)), case
        assert np.array_equal(_bits(hist_g), _bits(hist)) and np.array_equal(cnt_g, cnt), case          # reads, writes neither
        for e in range(n):                                     # zero rows exactly where no update step falls
            upd = {(int(cnt[e]) + i + 1) // p["every"] - int(cnt[e]) // p["every"] - 1 for i in range(steps)
                   if is_update(int(cnt[e]) + i + 1, **p)}
            for s in range(x.shape[1]):
                assert x[e, s].any() == (s in upd), (case, e, s)
        filled += int(x.any(2).sum())
        if case == "1x1_none":
            assert not x.any()
        if case == "1x1_update":
            assert x.all()
        if case == "3x25_slots":
            assert len({tuple(x[e].any(1)) for e in range(n)}) > 1, "the envs' slot patterns should differ"
    assert filled > 0
    # inactive envs get zero rows
    series, hist, cnt = case_inputs("19x37", p)
    active = np.arange(19) % 3 != 1
    x, _, _ = gpu_windows(ops, series, hist, cnt, active, lo=lo, scale=scale, **p)
    assert not x[~active].any() and np.array_equal(_bits(x), _bits(windows_ref(series, hist, cnt, active, lo=lo, scale=scale, **p)))


# ---------------------------------------------------------------------------------------------- 2. rule, synthetic pred
@pytest.mark.parametrize("pname", list(PARAMS))
def test_rule_is_the_restatement_bit_for_bit(ops, pname):
    p = PARAMS[pname]
    hits = misses = 0
    for case in CASES:
        series, hist, cnt = case_inputs(case, p)
        n, steps = series.shape
        pred = pred_for(pred_table(n, seed=steps), cnt, steps, p["every"])
        thr = np.full(n, np.nan)
        if case == "3x25_slots":
            thr[1:] = [61.5, 48.25]                                # envs past min_steps come in with a threshold
        want = rule_ref(series, hist, cnt, pred, thr, **p)
        got = gpu_rule(ops, series, hist, cnt, pred, thr, **p)
        _same(got, want, case)
        hits += int((want[0] >= 0).sum())
        misses += int((want[0] < 0).sum())
        if case == "1x1_none":
            assert np.isnan(got[3]).all() and got[0][0] == -1 and got[5][0] == 19
        if case == "1x1_update":
            assert got[3][0] == np.float64(pred[0, 0]) * FACTOR and got[5][0] == 20
    assert hits > 0 and misses > 0, (hits, misses)


def test_chunking_the_rule_changes_no_bit(ops):
    p = PARAMS["ref"]
    series, hist, cnt = case_inputs("19x37", p)
    n, steps = series.shape
    table = pred_table(n, seed=3)
    thr = np.full(n, np.nan)
    whole = gpu_rule(ops, series, hist, cnt, pred_for(table, cnt, steps, 10), thr, **p)
    _same(whole, rule_ref(series, hist, cnt, pred_for(table, cnt, steps, 10), thr, **p), "whole")
    assert (whole[0] >= 0).any() and (whole[0] < 0).any()
    for cuts in ((23, 14), (1,) * 37, (10, 10, 10, 7)):
        h, c, th = hist, cnt, thr
        stops, thrs, first, t0 = [], [], np.full(n, -1, np.int64), 0
        for k in cuts:
            f, st, to, th, h, c = gpu_rule(ops, np.ascontiguousarray(series[:, t0:t0 + k]), h, c, pred_for(table, c, k, 10), th, **p)
            first = np.where((first < 0) & (f >= 0), f + t0, first)
            stops.append(st)
            thrs.append(to)
            t0 += k
        assert np.array_equal(first, whole[0]), cuts
        assert np.array_equal(np.concatenate(stops, 1), whole[1]) and np.array_equal(_bits(np.concatenate(thrs, 1)), _bits(whole[2])), cuts
        assert np.array_equal(_bits(th), _bits(whole[3])) and np.array_equal(_bits(h), _bits(whole[4])) and np.array_equal(c, whole[5])


@pytest.mark.parametrize("D", [6, 8])
def test_column_of_the_records_is_read_in_place(ops, D):
    n, k, p = 11, 29, PARAMS["ref"]
    rng = np.random.RandomState(D)
    obs = torch.from_numpy((rng.uniform(0, 1, (n, k, D)) * rng.uniform(0.2, 1.0, (n, 1, 1))).astype(np.float32)).to(DEV)
    hist, cnt = np.zeros((n, 9), np.float32), np.zeros(n, np.int32)
    col = obs[:, :, 2]
    assert not col.is_contiguous() and col.stride() == (k * D, D)
    series = col.cpu().numpy()
    lo, scale = SCALER
    x, _, _ = gpu_windows(ops, col, hist, cnt, lo=lo, scale=scale, **p)
    assert x.any() and np.array_equal(_bits(x), _bits(windows_ref(series, hist, cnt, lo=lo, scale=scale, **p)))
    pred = pred_for(pred_table(n, seed=D), cnt, k, 10)
    got = gpu_rule(ops, col, hist, cnt, pred, np.full(n, np.nan), **p)
    _same(got, rule_ref(series, hist, cnt, pred, np.full(n, np.nan), **p), D)
    assert (got[0] >= 0).any()


def test_inactive_rows_and_nan_inputs(ops):
    n, steps, p = 8, 30, PARAMS["ref"]
    series = make_series(n, steps, seed=77)
    rng = np.random.RandomState(5)
    hist = rng.uniform(0, 1, (n, 9)).astype(np.float32)
    cnt = np.array([0, 23, 0, 5, 0, 40, 0, 0], np.int32)
    thr = np.array([np.nan, 55.0, np.nan, np.nan, np.nan, 70.0, np.nan, np.nan])
    active = np.array([1, 0, 1, 1, 0, 1, 1, 1], np.uint8)
    pred = pred_for(pred_table(n, seed=9), cnt, steps, 10)
    clean = gpu_rule(ops, series, hist, cnt, pred, thr, active, **p)
    _same(clean, rule_ref(series, hist, cnt, pred, thr, active, **p), "mask")
    off = active == 0
    assert (clean[0][off] == -1).all() and not clean[1][off].any()
    assert np.array_equal(_bits(clean[3][off]), _bits(thr[off])) and np.array_equal(_bits(clean[4][off]), _bits(hist[off]))
    assert np.array_equal(clean[5][off], cnt[off]) and np.array_equal(clean[5][~off], cnt[~off] + steps)
    # a NaN at (env 2, step 22) and (env 5, step 3): no hit on that step, nothing outside the env changes
    dirty_in = series.copy()
    dirty_in[2, 22] = np.nan
    dirty_in[5, 3] = np.nan
    dirty = gpu_rule(ops, dirty_in, hist, cnt, pred, thr, active, **p)
    _same(dirty, rule_ref(dirty_in, hist, cnt, pred, thr, active, **p), "nan")
    assert dirty[1][2, 22] == 0 and dirty[1][5, 3] == 0
    rest = np.ones(n, bool)
    rest[[2, 5]] = False
    for a, b in zip(dirty, clean):
        assert np.array_equal(_bits(a[rest]), _bits(b[rest]))
    # ... and a NaN inside a predictor window gives a NaN threshold, which is "no threshold": no hit until the next update
    x, _, _ = gpu_windows(ops, dirty_in, hist, cnt, active, **p)
    assert np.isnan(x[2, 2]).any() and not np.isnan(np.delete(x, 2, 0)[:, 2]).any()


# ---------------------------------------------------------------------------------------------- 3. through the predictor
def golden_scenario(ev):
    g = np.load(GOLD, allow_pickle=False)
    sd = {k[3:]: g[k] for k in g.files if k.startswith("sd/")}
    net = ev.ConcentrationThresholdPredictor(hidden_size=32, device=DEV)
    net.load_state_dict(sd)
    lo, hi = float(g["scaler_params"].min()), float(g["scaler_params"].max())
    return net, eo.ThresholdPredictorOracle(sd), (g["traj"] / 100.0).astype(np.float32), lo, hi - lo, g["stop_at"]


def seeded_predictor(ev, device):
    """tests/test_gpu_eval.py's hidden-64 predictor: thresholds inside the plume's concentration range"""
    pred = ev.ConcentrationThresholdPredictor(hidden_size=64, device=device, seed=4)
    pred.fc["fc.4.bias"].fill_(18.0)
    pred.fc["fc.4.weight"].mul_(6.0)
    return pred


def seeded_series(n=19, steps=57, seed=11):
    """concentrations / 100 that drift upwards through the seeded predictor's thresholds (about 17) at an env's own pace, or never"""
    rng = np.random.RandomState(seed)
    slope = rng.uniform(0.0, 0.008, (n, 1)) * (np.arange(n) % 4 != 2)[:, None]
    base = rng.uniform(0.02, 0.10, (n, 1))
    return (base + slope * np.arange(steps)[None] + rng.uniform(-0.01, 0.01, (n, steps))).clip(0).astype(np.float32)


def _cpu_sd(model):
    return {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}


def oracle_chunk(onet, series, lo, scale, p):
    n, steps = series.shape
    hist, cnt = np.zeros((n, p["window"] - 1), np.float32), np.zeros(n, np.int32)
    x = windows_ref(series, hist, cnt, lo=lo, scale=scale, **p)
    pred = onet(x.reshape(-1, p["window"], 1)).numpy().reshape(n, -1)
    met = []
    first, stop, thr_out, _, _, _ = rule_ref(series, hist, cnt, pred, np.full(n, np.nan), met=met, **p)
    return first, stop, thr_out, live_margin(met, first)


def device_chunks(ops, net, series, lo, scale, p, cuts):
    n = series.shape[0]
    s = torch.from_numpy(series).to(DEV)
    hist = torch.zeros(n, p["window"] - 1, device=DEV)
    cnt = torch.zeros(n, dtype=torch.int32, device=DEV)
    thr = torch.full((n,), float("nan"), dtype=torch.float64, device=DEV)
    first, stops, thrs, t0 = np.full(n, -1, np.int64), [], [], 0
    for k in cuts:
        part = s[:, t0:t0 + k]                                      # a strided view
        x = ops.threshold_windows(part, hist, cnt, lo=lo, scale=scale, **p)
        pred = net(x.reshape(-1, p["window"], 1)).reshape(n, -1).contiguous()
        f, st, to = ops.threshold_rule(part, hist, cnt, pred, thr, **p)
        f = f.cpu().numpy()
        first = np.where((first < 0) & (f >= 0), f + t0, first)
        stops.append(st.cpu().numpy())
        thrs.append(to.cpu().numpy())
        t0 += k
    return first, np.concatenate(stops, 1), np.concatenate(thrs, 1)


@pytest.mark.parametrize("which", ["golden_h32", "seeded_h64"])
def test_thresholds_and_decisions_match_the_f32_oracle(ops, ev, which):
    p = REFERENCE
    if which == "golden_h32":
        net, onet, series, lo, scale, stop_at = golden_scenario(ev)
    else:
        net = seeded_predictor(ev, DEV)
        onet, series, lo, scale, stop_at = eo.ThresholdPredictorOracle(_cpu_sd(net)), seeded_series(), 0.0, 100.0, None
    n, steps = series.shape
    first_w, stop_w, thr_w, margin = oracle_chunk(onet, series, lo, scale, p)
    thr_max = np.nanmax(thr_w)
    assert margin > margin_needed(thr_max), (which, margin, margin_needed(thr_max))
    assert (first_w >= 0).any() and (first_w < 0).any(), first_w
    if stop_at is not None:
        assert np.array_equal(np.where(first_w >= 0, first_w + 1, -1), stop_at)
    for cuts in ((steps,), (50, steps - 50), (17,) * (steps // 17) + ((steps % 17,) if steps % 17 else ())):
        first, stop, thr = device_chunks(ops, net, series, lo, scale, p, cuts)
        assert np.array_equal(first, first_w), (which, cuts, first, first_w)
        worst = 0.0
        for e in range(n):
            live = steps if first_w[e] < 0 else first_w[e] + 1
            assert np.array_equal(stop[e, :live], stop_w[e, :live]), (which, cuts, e)
            assert np.array_equal(np.isnan(thr[e]), np.isnan(thr_w[e]))
            ok = ~np.isnan(thr_w[e])
            err = np.abs(thr[e][ok] - thr_w[e][ok])
            assert (err <= tol(thr_w[e][ok] / FACTOR)).all(), (which, cuts, e, err.max())
            worst = max(worst, err.max() if ok.any() else 0.0)
        print(f"{which} cuts {cuts}: max |thr err| {worst:.3g} (tol {tol(thr_max / FACTOR):.3g}), oracle margin {margin:.3g}")


# ---------------------------------------------------------------------------------------------- 4. episodes
class MarginController(eo.ThresholdControllerOracle):
    """The oracle's controller, recording every distance its rule compares (all of an oracle episode's steps are live)."""

    def __init__(self, *a, met=None, **k):
        super().__init__(*a, **k)
        self.met = met

    def should_stop(self, current_conc, step_count):
        out = super().should_stop(current_conc, step_count)
        if step_count >= self.min_activate_steps and self.current_threshold is not None:
            self.met.append((abs(current_conc - self.current_threshold), abs(np.mean(self.conc_buffer) - self.current_threshold),
                             self.current_threshold))
        return out


def _met_margin(met):
    m = np.asarray(met)
    return float(m[:, :2].min()), margin_needed(float(m[:, 2].max()))


def mlp_scenario(ev, device):
    """tests/test_gpu_eval.py::test_vectorised_greedy_evaluation_matches_oracle_episodes': N = 12, 120 steps, v2.0, scaler (0, 100)"""
    from uavppo.policy import MLPActorCritic
    N, LIM = 12, 120
    bank = FieldBank.from_seed(N, "v2.0", seed=9)
    pol = MLPActorCritic(6, 5, device=device, seed=8)
    pol.views["head.weight"][:5].mul_(40.0)
    return N, LIM, bank, pol, seeded_predictor(ev, device), np.random.RandomState(1).randn(LIM, N, 2)


def mlp_env(bank, N):
    from uavppo.vec_env import VecMethaneEnv
    return VecMethaneEnv(N, "v2.0", DEV, seed=3, bank=bank.interleaved(), bank_sources=bank.sources)


def mlp_oracle_episodes(N, LIM, bank, pol, pred, noise):
    p = {k: v.detach().cpu() for k, v in pol.named_views().items()}
    onet = eo.ThresholdPredictorOracle(_cpu_sd(pred))
    ora = OracleVecEnv(N, bank, "v2.0", radius=50.0)
    ora.reset()
    steps, stopped, devs, met = [], [], [], []
    for i, e in enumerate(ora.envs):
        octl = MarginController(onet, np.array((0.0, 100.0)), met=met)
        state, traj, t, done, st = e.obs(), [], 0, False, False
        while not done and t < LIM:
            with torch.no_grad():
                probs, _, _ = po.mlp_forward(p, torch.from_numpy(state)[None])
            state, _, done, _r, _i = e.step(int(torch.argmax(probs)), noise[t, i])
            cur = float(state[2]) * 100.0
            traj.append(cur)
            t += 1
            if t % 10 == 0:
                octl.update_threshold(traj)
            if octl.should_stop(cur, t):
                st, done = True, True
        steps.append(t)
        stopped.append(st)
        devs.append(float(np.linalg.norm(np.asarray(e.pos, np.float64) - np.asarray(e.source, np.float64))))
    return np.asarray(steps), np.asarray(stopped), np.asarray(devs), met


def lstm_oracle_episodes(pol, pred, bank, N, LIM, noise):
    onet = eo.ThresholdPredictorOracle(_cpu_sd(pred))
    met = []

    def stop():                                           # evaluate_with_lstm.py:87-93 for one env's episode
        o = MarginController(onet, np.array((0.0, 100.0)), met=met)

        def rule(traj, t):
            if t % 10 == 0:
                o.update_threshold(traj)
            return o.should_stop(traj[-1], t)
        return rule

    steps, stopped, devs, _, gap = _oracle_lstm(pol, bank, "v2.0", N, LIM, noise, stop=stop)
    return steps, stopped, devs, met, gap


def _controller(ev, pred, N):
    return ev.ThresholdController(pred, (0.0, 100.0), N, device=DEV)


def test_evaluate_device_rule_matches_oracle_episodes_mlp(ev):
    N, LIM, bank, pol, pred, noise = mlp_scenario(ev, DEV)
    steps, stopped, devs, met = mlp_oracle_episodes(N, LIM, bank, pol, pred, noise)
    margin, need = _met_margin(met)
    assert margin > need, (margin, need)
    assert 0 < stopped.sum() < N, stopped                  # some envs are stopped by the rule, some are not
    ctl = _controller(ev, pred, N)
    got = ev.evaluate(pol, mlp_env(bank, N), ctl, noise=torch.from_numpy(noise).to(DEV), max_steps=LIM, fused=True,
                      threshold_device=True)
    _agree(got, steps, stopped, devs)
    thr = ctl.current_threshold
    assert thr.dtype == torch.float64 and thr.shape == (N,) and bool(torch.isnan(thr[torch.from_numpy(steps < 20).to(DEV)]).all())
    print(f"{stopped.sum()} of {N} episodes stopped by the rule; oracle margin {margin:.3g} (needed {need:.3g})")


def test_evaluate_device_rule_matches_oracle_episodes_lstm64(ev):
    N, LIM = 37, 200                                      # test_gpu_greedy_eval's h = 64 scenario with the controller
    noise = np.random.RandomState(64).randn(LIM, N, 2)
    bank, env = _bank_env(N, "v2.0", 94, 3)
    pol = _lstm_policy(64, seed=6, bias=TOWARDS)
    pred = seeded_predictor(ev, DEV)
    steps, stopped, devs, met, gap = lstm_oracle_episodes(pol, pred, bank, N, LIM, noise)
    margin, need = _met_margin(met)
    assert gap > GAP and margin > need, (gap, margin, need)
    assert 0 < stopped.sum() < N, stopped
    got = ev.evaluate(pol, env, _controller(ev, pred, N), noise=torch.from_numpy(noise).to(DEV), max_steps=LIM, fused=True,
                      threshold_device=True)
    _agree(got, steps, stopped, devs)


def test_same_metrics_through_every_route(ev):
    N, LIM, bank, pol, pred, noise = mlp_scenario(ev, DEV)
    nz = torch.from_numpy(noise).to(DEV)
    call = lambda o: pol.heads(o.contiguous())[:, :5]
    run = lambda policy, **kw: ev.evaluate(policy, mlp_env(bank, N), _controller(ev, pred, N), noise=nz, max_steps=LIM, **kw)
    outs = [run(pol, fused=True, threshold_device=True),                    # fused device rule, the default chunk (50)
            run(pol, fused=True, threshold_device=True, chunk=17),
            run(pol, fused=True),                                           # fused replay (the default)
            run(pol, fused=True, chunk=17),
            run(pol, fused=False, threshold_device=True),                   # step-wise device rule
            run(call, threshold_device=True),
            run(call)]
    for o in outs[1:]:
        _equal(outs[0], o)
    assert 0 < outs[0]["stopped_early"].sum() < N


def test_lstm_policy_routes_agree(ev):
    N, LIM = 37, 200
    nz = torch.from_numpy(np.random.RandomState(64).randn(LIM, N, 2)).to(DEV)
    pol = _lstm_policy(64, seed=6, bias=TOWARDS)
    pred = seeded_predictor(ev, DEV)
    outs = []
    for kw in ({"threshold_device": True}, {"threshold_device": True, "chunk": 17}, {}):
        _, env = _bank_env(N, "v2.0", 94, 3)
        outs.append(ev.evaluate(pol, env, _controller(ev, pred, N), noise=nz, max_steps=LIM, fused=True, **kw))
    for o in outs[1:]:
        _equal(outs[0], o)
    assert 0 < outs[0]["stopped_early"].sum() < N


def peak_predictor(ev, device):
    """A PPOV2.1 predictor that, on the h = 64 LSTM scenario, fires before the threshold rule for some envs, with it for some, after
    it or never for others (settled on the CPU oracle: smallest |stop_prob - 0.8| met while an episode is live 1.6e-3, against the
    2e-5 between the predictor's two f32 routes)."""
    pred = ev.PeakAndStopPredictor(device=device, seed=19)
    pred.heads_w[1].mul_(12.0)
    pred.lstm.p["weight_ih_l0"].mul_(60.0)
    return pred


def test_both_rules_on_the_device_and_each_beside_the_others_replay(ev):
    """The live steps of these episodes are a subset of test_evaluate_device_rule_matches_oracle_episodes_lstm64's (the second rule
    only ends episodes earlier), whose oracle asserts the threshold rule's margin."""
    N, LIM = 37, 200
    nz = torch.from_numpy(np.random.RandomState(64).randn(LIM, N, 2)).to(DEV)
    pol = _lstm_policy(64, seed=6, bias=TOWARDS)
    pred, peak = seeded_predictor(ev, DEV), peak_predictor(ev, DEV)

    def run(**kw):
        _, env = _bank_env(N, "v2.0", 94, 3)
        return ev.evaluate(pol, env, _controller(ev, pred, N), noise=nz, max_steps=LIM, **kw)

    outs = {name: run(peak_stop=peak, **dict({"fused": True}, **kw)) for name, kw in (
        ("replay", {}), ("both", {"threshold_device": True, "peak_stop_device": True}),
        ("both_17", {"threshold_device": True, "peak_stop_device": True, "chunk": 17}),
        ("thr_dev", {"threshold_device": True}), ("peak_dev", {"peak_stop_device": True}),
        ("both_stepwise", {"threshold_device": True, "peak_stop_device": True, "fused": False}))}
    want = outs["replay"]
    for name, got in outs.items():
        assert sorted(got) == sorted(want)
        for k in ("steps", "stopped_early", "deviations", "success"):
            assert np.array_equal(got[k], want[k]), (name, k)
        assert np.allclose(got["peak_pred"], want["peak_pred"], rtol=0, atol=PEAK_TOL, equal_nan=True), name
    _equal(outs["both"], outs["both_17"])
    # both rules take part: the peak rule ends some episodes (peak_pred recorded), the threshold rule alone others, some run on
    by_peak = ~np.isnan(want["peak_pred"])
    assert by_peak.any() and (want["stopped_early"] & ~by_peak).any() and not want["stopped_early"].all(), (by_peak, want["stopped_early"])
    assert not np.array_equal(want["steps"], run(fused=True)["steps"])                    # ... and the peak rule changes the outcome


# ---------------------------------------------------------------------------------------------- 5. main(threshold_device=True)
@pytest.mark.parametrize("policy", ["lstm", "mlp"])
def test_main_runs_the_rule_on_the_device(ev, tmp_path, monkeypatch, policy):
    """main()'s keyword reaches evaluate() on both of its routes (policy object -> fused chunks, logits function -> step-wise).  The
    predictor's output bias puts every threshold far below (everything stops at step 20, the first with a threshold) or far above
    (nothing is stopped) any concentration, so the two rules' decisions cannot hinge on rounding."""
    from model import PPOActorCritic
    from uavppo.policy import LSTMActorCritic
    model_dir = tmp_path / "model"
    os.makedirs(model_dir)
    pol = LSTMActorCritic(6, 64, 1, device="cpu", seed=11) if policy == "lstm" else PPOActorCritic(6, 5, device=DEV)
    torch.save({k: v.detach().cpu() for k, v in pol.state_dict().items()}, str(model_dir / "ppo_successful_models.pth"))
    np.save(str(model_dir / "scaler_params.npy"), np.array([0.0, 100.0]))
    monkeypatch.chdir(tmp_path)
    for bias, all_stop in ((-1e6, True), (1e6, False)):
        pred = ev.ConcentrationThresholdPredictor(device="cpu", seed=2)
        pred.fc["fc.4.bias"].fill_(bias)
        torch.save(pred.state_dict(), str(model_dir / "lstm_threshold_predictor.pth"))
        host = ev.main(num_envs=32, model_dir=str(model_dir), device=DEV, policy=policy)
        dev = ev.main(num_envs=32, model_dir=str(model_dir), device=DEV, policy=policy, threshold_device=True)
        _equal(host, dev)
        live = dev["steps"] >= 20                                                  # episodes the env had not ended before step 20
        assert live.any() and np.array_equal(dev["stopped_early"], live if all_stop else np.zeros(32, bool))
        assert (dev["steps"][live] == 20).all() if all_stop else (dev["steps"] > 20).any()
