"""uav_peak_stop_scan (csrc/peak_stop.hip: the PPOV2.1 PeakAndStopPredictor over every sliding window of a chunk, the 0.8 rule
and the first hit per env on the device) and evaluate(..., peak_stop_device=True) on top of it.  -m gpu.

The oracle is torch's own nn.LSTM(1, 32, batch_first=True) + two nn.Linear in float64 with the predictor's weights; episodes
are oracle.eval_oracle.stop_rule_v21 around it.  Values are compared to 2e-5 absolute, the bound tests/test_gpu_eval.py accepts
between this predictor on the GPU and its CPU restatement.  Decisions (prob > 0.8) are compared exactly, which is sound because
every scenario asserts on the oracle's side that no f64 probability it meets lies within 1e-4 (five times the tolerance) of 0.8."""
import numpy as np
import pytest
import torch

from oracle import eval_oracle as eo
from oracle import ppo_oracle as po
from oracle.env_oracle import OracleVecEnv
from test_gpu_greedy_eval import GAP, TOWARDS, _agree, _bank_env, _equal, _lstm_policy, _oracle_lstm, ev  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 2e-5
MARGIN = 1e-4
PROB_MIN = 0.8


# ---------------------------------------------------------------------------------------------- the f64 oracle
class F64Predictor:
    """PeakAndStopPredictor's state_dict in torch's own float64 modules; `met` collects every stop probability it returned."""

    def __init__(self, sd):
        sd = {k: torch.as_tensor(np.asarray(v)).double() for k, v in sd.items()}
        H = sd["lstm.weight_hh_l0"].shape[1]
        self.lstm = torch.nn.LSTM(1, H, batch_first=True).double()
        self.lstm.load_state_dict({k[5:]: v for k, v in sd.items() if k.startswith("lstm.")})
        self.fc_peak, self.fc_stop = torch.nn.Linear(H, 1).double(), torch.nn.Linear(H, 1).double()
        self.fc_peak.load_state_dict({"weight": sd["fc_peak.weight"], "bias": sd["fc_peak.bias"]})
        self.fc_stop.load_state_dict({"weight": sd["fc_stop.0.weight"], "bias": sd["fc_stop.0.bias"]})
        self.met = []

    @torch.no_grad()
    def __call__(self, x):
        x = torch.as_tensor(np.asarray(x)).double()
        if x.dim() == 2:
            x = x.unsqueeze(-1)
        _, (hn, _) = self.lstm(x)
        peak, prob = self.fc_peak(hn[0]).squeeze(-1), torch.sigmoid(self.fc_stop(hn[0])).squeeze(-1)
        self.met.extend(prob.reshape(-1).tolist())
        return peak, prob

    def margin(self):
        p = np.asarray(self.met)
        p = p[~np.isnan(p)]
        return np.abs(p - PROB_MIN).min() if p.size else np.inf


def make_predictor(ev, device, seed=10):
    """A predictor whose rule fires on some windows and not on others: the decisive stop head of the existing tests, and an input
    gain that makes the LSTM respond to concentrations / 100 of a few hundredths (with the default initialisation stop_prob hardly
    moves with the input, so the rule would fire always or never)."""
    pred = ev.PeakAndStopPredictor(device=device, seed=seed)
    pred.heads_w[1].mul_(12.0)
    pred.lstm.p["weight_ih_l0"].mul_(250.0)
    return pred


def _cpu_sd(pred):
    return {k: v.detach().cpu().numpy() for k, v in pred.state_dict().items()}


def make_series(n, steps, seed):
    """Uniform random concentrations; each env has its own level (every fourth a very low one), so that windows fall on both sides
    of the rule."""
    rng = np.random.RandomState(seed)
    level = rng.uniform(0.05, 1.0, (n, 1)) * np.where(np.arange(n) % 4 == 1, 0.01, 1.0)[:, None]
    return (rng.uniform(0.0, 1.0, (n, steps)) * level).astype(np.float32)


def make_hist(n, window, cnt, seed):
    rng = np.random.RandomState(seed + 1000)
    hist = (rng.uniform(0.0, 1.0, (n, window - 1)) * rng.uniform(0.05, 1.0, (n, 1))).astype(np.float32)
    return hist, np.broadcast_to(np.asarray(cnt, np.int32), (n,)).copy()


def oracle_scan(onet, series, hist, cnt, window, active=None):
    """uav_peak_stop_scan restated: (peak, prob f64 [n, steps] with NaN in invalid / inactive slots, first_hit, hist, cnt on exit)."""
    n, steps = series.shape
    active = np.ones(n, bool) if active is None else np.asarray(active, bool)
    peak, prob = np.full((n, steps), np.nan), np.full((n, steps), np.nan)
    seqs = [np.concatenate([hist[e, :cnt[e]], series[e]]) for e in range(n)]
    slots = [(e, i) for e in range(n) for i in range(steps) if active[e] and cnt[e] + i + 1 >= window]
    if slots:
        x = np.stack([seqs[e][cnt[e] + i + 1 - window:cnt[e] + i + 1] for e, i in slots])
        pk, pr = onet(x[:, :, None])
        for (e, i), a, b in zip(slots, pk.numpy(), pr.numpy()):
            peak[e, i], prob[e, i] = a, b
    first = np.full(n, -1, np.int32)
    hist_out, cnt_out = hist.copy(), cnt.copy()
    for e in range(n):
        if not active[e]:
            continue
        hits = np.nonzero(prob[e] > PROB_MIN)[0]          # NaN > 0.8 is False
        first[e] = hits[0] if hits.size else -1
        tail = seqs[e][-(window - 1):] if window > 1 else seqs[e][:0]
        cnt_out[e] = len(tail)
        hist_out[e, :len(tail)] = tail
    return peak, prob, first, hist_out, cnt_out


# (n, steps, hist_cnt per window): none, full, partly filled (some windows valid, some not), none
SCAN_CASES = {"19x37": (19, 37, lambda w: 0), "1x1_full": (1, 1, lambda w: w - 1),
              "3x5_partial": (3, 5, lambda w: [w - 3, w - 5, w - 1]), "16x16": (16, 16, lambda w: 0)}


def scan_inputs(case, window):
    n, steps, cnt = SCAN_CASES[case]
    series = make_series(n, steps, seed=n * 100 + steps + window)
    hist, cnt = make_hist(n, window, cnt(window), seed=n + window)
    return series, hist, cnt


def gpu_scan(ops, pred, window, series, hist, cnt, active=None, **kw):
    """-> first_hit, peak, prob, hist, cnt as numpy; series may be a (strided) device tensor already"""
    s = series if torch.is_tensor(series) else torch.from_numpy(series).to(DEV)
    h, c = torch.from_numpy(hist).to(DEV), torch.from_numpy(cnt).to(DEV)
    a = None if active is None else torch.from_numpy(np.asarray(active, np.uint8)).to(DEV)
    first, peak, prob = ops.peak_stop_scan(pred.flat_params(), 32, window, s, h, c, active=a, **kw)
    return first.cpu().numpy(), peak.cpu().numpy(), prob.cpu().numpy(), h.cpu().numpy(), c.cpu().numpy()


@pytest.fixture(scope="module")
def ops():
    from uavppo import ops as o
    return o


@pytest.fixture(scope="module")
def pred(ev):
    return make_predictor(ev, DEV)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---------------------------------------------------------------------------------------------- 1. scan vs the f64 oracle
@pytest.mark.parametrize("window", [20, 7])
def test_scan_matches_f64_oracle(ops, pred, window):
    hits = misses = 0
    for case in SCAN_CASES:
        series, hist, cnt = scan_inputs(case, window)
        onet = F64Predictor(_cpu_sd(pred))
        peak_w, prob_w, first_w, hist_w, cnt_w = oracle_scan(onet, series, hist, cnt, window)
        assert onet.margin() > MARGIN, (case, window, onet.margin())
        first, peak, prob, hist_g, cnt_g = gpu_scan(ops, pred, window, series, hist, cnt)
        valid = ~np.isnan(prob_w)
        err_peak = np.abs(peak[valid] - peak_w[valid]).max() if valid.any() else 0.0
        err_prob = np.abs(prob[valid] - prob_w[valid]).max() if valid.any() else 0.0
        print(f"{case} window {window}: {valid.sum()} valid windows, max |peak err| {err_peak:.3g}, max |prob err| {err_prob:.3g}")
        assert np.isnan(peak[~valid]).all() and np.isnan(prob[~valid]).all(), case
        assert np.isfinite(peak[valid]).all() and err_peak <= TOL and err_prob <= TOL, (case, err_peak, err_prob)
        assert np.array_equal(first, first_w), (case, first, first_w)
        assert np.array_equal(_bits(hist_g), _bits(hist_w)) and np.array_equal(cnt_g, cnt_w), case
        hits += int((prob_w[valid] > PROB_MIN).sum())
        misses += int((prob_w[valid] <= PROB_MIN).sum())
        if case == "3x5_partial":
            assert valid.any(1).all() and not valid.all(), "the partly filled case must mix valid and invalid windows"
        if case == "19x37" and window == 20:
            assert (first_w >= 0).any() and (first_w < 0).any(), first_w
    assert hits > 0 and misses > 0, (hits, misses)


# ---------------------------------------------------------------------------------------------- 2. chunk invariance
def test_chunking_the_scan_changes_no_bit(ops, pred):
    window, (n, steps) = 20, (19, 37)
    series, hist, cnt = scan_inputs("19x37", window)
    whole = gpu_scan(ops, pred, window, series, hist, cnt)
    assert (whole[0] >= 0).any()
    for cuts in ((23, 14), (1,) * 37):
        h, c = hist, cnt
        peaks, probs, first, t0 = [], [], np.full(n, -1, np.int64), 0
        for k in cuts:
            f, pk, pr, h, c = gpu_scan(ops, pred, window, np.ascontiguousarray(series[:, t0:t0 + k]), h, c)
            first = np.where((first < 0) & (f >= 0), f + t0, first)
            peaks.append(pk)
            probs.append(pr)
            t0 += k
        assert np.array_equal(_bits(np.concatenate(peaks, 1)), _bits(whole[1])), cuts
        assert np.array_equal(_bits(np.concatenate(probs, 1)), _bits(whole[2])), cuts
        assert np.array_equal(first, whole[0]), cuts
        assert np.array_equal(_bits(h), _bits(whole[3])) and np.array_equal(c, whole[4]), cuts
    again = gpu_scan(ops, pred, window, series, hist, cnt)          # and the same call twice: the same bits
    for a, b in zip(whole, again):
        assert np.array_equal(_bits(a), _bits(b))


# ---------------------------------------------------------------------------------------------- 3. strided input
@pytest.mark.parametrize("D", [6, 8])
def test_column_of_the_records_is_read_in_place(ops, pred, D):
    n, k, window = 11, 29, 20
    obs = torch.from_numpy(np.random.RandomState(D).uniform(0, 1, (n, k, D)).astype(np.float32)).to(DEV)
    hist, cnt = make_hist(n, window, 0, seed=D)
    col = obs[:, :, 2]
    assert not col.is_contiguous() and col.stride() == (k * D, D)
    got = gpu_scan(ops, pred, window, col, hist, cnt)
    want = gpu_scan(ops, pred, window, col.contiguous(), hist, cnt)
    assert np.isfinite(got[2]).any()
    for a, b in zip(got, want):
        assert np.array_equal(a, b, equal_nan=True)
    assert np.array_equal(_bits(got[1]), _bits(want[1])) and np.array_equal(_bits(got[2]), _bits(want[2]))


# ---------------------------------------------------------------------------------------------- 4. active mask, NaN
def test_inactive_rows_and_nan_inputs(ops, pred):
    n, steps, window = 8, 30, 20
    series = make_series(n, steps, seed=77)
    hist, cnt = make_hist(n, window, [0, 19, 0, 5, 0, 19, 0, 0], seed=5)
    active = np.array([1, 0, 1, 1, 0, 1, 1, 1], np.uint8)
    clean = gpu_scan(ops, pred, window, series, hist, cnt, active)
    off = active == 0
    assert (clean[0][off] == -1).all() and np.isnan(clean[1][off]).all() and np.isnan(clean[2][off]).all()
    assert np.array_equal(_bits(clean[3][off]), _bits(hist[off])) and np.array_equal(clean[4][off], cnt[off])
    assert np.isfinite(clean[2][~off][:, -1]).all() and (clean[4][~off] == window - 1).all()
    # a NaN at (env 2, step 25) and at (env 5, step 3): NaN in the windows that hold it, the same bits everywhere else
    dirty_in = series.copy()
    dirty_in[2, 25] = np.nan
    dirty_in[5, 3] = np.nan
    dirty = gpu_scan(ops, pred, window, dirty_in, hist, cnt, active)
    holds = np.zeros((n, steps), bool)
    holds[2, 25:] = True                                    # steps 25 .. 29: windows [i - 19, i] that contain step 25
    holds[5, 3:3 + window] = True                           # env 5 comes in with a full history: every window from step 3 to 22
    assert np.isnan(dirty[1][holds]).all() and np.isnan(dirty[2][holds]).all()
    for k in (1, 2):
        assert np.array_equal(_bits(dirty[k][~holds]), _bits(clean[k][~holds]))
    for e in (2, 5):                                         # no hit inside the NaN windows
        want = np.nonzero((clean[2][e] > PROB_MIN) & ~holds[e])[0]
        assert dirty[0][e] == (want[0] if want.size else -1)
    rest = np.ones(n, bool)
    rest[[2, 5]] = False
    assert np.array_equal(dirty[0][rest], clean[0][rest])


# ---------------------------------------------------------------------------------------------- 5. evaluate vs oracle episodes
def mlp_scenario(ev, device):
    """tests/test_gpu_eval.py::test_vectorised_greedy_evaluation_v21_stop_rule_matches_oracle's: N = 10, 90 steps, v2.1."""
    from oracle.env_oracle import FieldBank
    from uavppo.policy import MLPActorCritic
    N, LIM = 10, 90
    bank = FieldBank.from_seed(N, "v2.1", seed=21)
    pol = MLPActorCritic(6, 5, device=device, seed=12)
    pol.views["head.weight"][:5].mul_(40.0)
    return N, LIM, bank, pol, make_predictor(ev, device), np.random.RandomState(4).randn(LIM, N, 2)


def mlp_env(bank, N):
    from uavppo.vec_env import VecMethaneEnv
    return VecMethaneEnv(N, "v2.1", DEV, seed=5, bank=bank.interleaved(), bank_sources=bank.sources)


def mlp_oracle_episodes(N, LIM, bank, pol, onet, noise):
    p = {k: v.detach().cpu() for k, v in pol.named_views().items()}
    ora = OracleVecEnv(N, bank, "v2.1", radius=50.0)
    ora.reset()
    steps, stopped, devs, peaks = [], [], [], []
    for i, e in enumerate(ora.envs):
        state, traj, t, done, st, pk = e.obs(), [], 0, False, False, np.nan
        while not done and t < LIM:
            with torch.no_grad():
                probs, _, _ = po.mlp_forward(p, torch.from_numpy(state)[None])
            state, _, done, _r, _i = e.step(int(torch.argmax(probs)), noise[t, i])
            traj.append(float(state[2]) * 100.0)
            t += 1
            hit, peak = eo.stop_rule_v21(onet, traj)
            if hit:
                st, done, pk = True, True, peak
        steps.append(t)
        stopped.append(st)
        peaks.append(pk)
        devs.append(float(np.linalg.norm(np.asarray(e.pos, np.float64) - np.asarray(e.source, np.float64))))
    return np.asarray(steps), np.asarray(stopped), np.asarray(devs), np.asarray(peaks)


def lstm_oracle_episodes(pol, bank, N, LIM, noise, onet):
    """test_gpu_greedy_eval's f64 LSTM episodes with the v2.1 rule; the peak of the step that stopped each episode"""
    peaks = []

    def stop():
        peaks.append(np.nan)

        def rule(traj, t):
            hit, peak = eo.stop_rule_v21(onet, traj)
            if hit:
                peaks[-1] = peak
            return hit
        return rule

    steps, stopped, devs, _, gap = _oracle_lstm(pol, bank, "v2.1", N, LIM, noise, stop=stop)
    return steps, stopped, devs, np.asarray(peaks), gap


def _check_episodes(got, steps, stopped, devs, peaks):
    _agree(got, steps, stopped, devs)
    assert 0 < stopped.sum() < len(stopped), stopped
    assert np.isnan(got["peak_pred"][~stopped]).all()
    err = np.abs(got["peak_pred"][stopped] - peaks[stopped]).max()
    print(f"{stopped.sum()} of {len(stopped)} episodes stopped by the rule, max |peak_pred err| {err:.3g}")
    assert err <= TOL, err


def test_evaluate_device_rule_matches_oracle_episodes_mlp(ev):
    N, LIM, bank, pol, pred, noise = mlp_scenario(ev, DEV)
    onet = F64Predictor(_cpu_sd(pred))
    steps, stopped, devs, peaks = mlp_oracle_episodes(N, LIM, bank, pol, onet, noise)
    assert onet.margin() > MARGIN, onet.margin()
    got = ev.evaluate(pol, mlp_env(bank, N), None, peak_stop=pred, noise=torch.from_numpy(noise).to(DEV), max_steps=LIM,
                      fused=True, peak_stop_device=True)
    _check_episodes(got, steps, stopped, devs, peaks)


def test_evaluate_device_rule_matches_oracle_episodes_lstm64(ev):
    N, LIM = 37, 200                                      # test_gpu_greedy_eval's h = 64 scenario on the v2.1 env
    noise = np.random.RandomState(7).randn(LIM, N, 2)
    bank, env = _bank_env(N, "v2.1", 94, 3)
    pol = _lstm_policy(64, seed=6, bias=TOWARDS)
    pred = make_predictor(ev, DEV)
    onet = F64Predictor(_cpu_sd(pred))
    steps, stopped, devs, peaks, gap = lstm_oracle_episodes(pol, bank, N, LIM, noise, onet)
    assert gap > GAP and onet.margin() > MARGIN, (gap, onet.margin())
    got = ev.evaluate(pol, env, None, peak_stop=pred, noise=torch.from_numpy(noise).to(DEV), max_steps=LIM, fused=True,
                      peak_stop_device=True)
    _check_episodes(got, steps, stopped, devs, peaks)


# ---------------------------------------------------------------------------------------------- 6. every route, same metrics
def test_same_metrics_through_every_route(ev):
    N, LIM, bank, pol, pred, noise = mlp_scenario(ev, DEV)
    nz = torch.from_numpy(noise).to(DEV)
    kw = dict(peak_stop=pred, noise=nz, max_steps=LIM)
    call = lambda o: pol.heads(o.contiguous())[:, :5]
    dev = [ev.evaluate(pol, mlp_env(bank, N), fused=True, chunk=23, peak_stop_device=True, **kw),
           ev.evaluate(pol, mlp_env(bank, N), fused=True, chunk=90, peak_stop_device=True, **kw),
           ev.evaluate(pol, mlp_env(bank, N), fused=True, peak_stop_device=True, **kw),          # the default chunk (50)
           ev.evaluate(call, mlp_env(bank, N), peak_stop_device=True, **kw),
           ev.evaluate(pol, mlp_env(bank, N), fused=False, peak_stop_device=True, **kw)]
    for o in dev[1:]:
        _equal(dev[0], o)
    host = ev.evaluate(pol, mlp_env(bank, N), fused=True, chunk=23, **kw)          # the host replay (the default)
    assert sorted(host) == sorted(dev[0])
    for k in ("steps", "stopped_early", "deviations", "success"):
        assert np.array_equal(host[k], dev[0][k]), k
    st = host["stopped_early"]
    assert 0 < st.sum() < N
    assert np.array_equal(np.isnan(host["peak_pred"]), np.isnan(dev[0]["peak_pred"])) and np.isnan(host["peak_pred"][~st]).all()
    assert np.abs(host["peak_pred"][st] - dev[0]["peak_pred"][st]).max() <= TOL


def test_device_rule_beside_a_threshold_controller(ev):
    """Both controllers at once: the V2.0 controller keeps its replay loop, the V2.1 rule comes from the scan's per-step values."""
    N, LIM, bank, pol, pred, noise = mlp_scenario(ev, DEV)
    nz = torch.from_numpy(noise).to(DEV)
    outs = []
    for kw in ({}, {"peak_stop_device": True}, {"peak_stop_device": True, "chunk": 90}):
        tp = ev.ConcentrationThresholdPredictor(hidden_size=64, device=DEV, seed=4)
        tp.fc["fc.4.bias"].fill_(18.0)
        tp.fc["fc.4.weight"].mul_(6.0)
        ctl = ev.ThresholdController(tp, (0.0, 100.0), N, device=DEV)
        outs.append(ev.evaluate(pol, mlp_env(bank, N), ctl, peak_stop=pred, noise=nz, max_steps=LIM, fused=True, **kw))
    _equal(outs[1], outs[2])
    for k in ("steps", "stopped_early", "deviations"):
        assert np.array_equal(outs[0][k], outs[1][k]), k
    assert np.allclose(outs[0]["peak_pred"], outs[1]["peak_pred"], rtol=0, atol=TOL, equal_nan=True)


# ---------------------------------------------------------------------------------------------- 7. refusal
def test_a_predictor_the_kernel_does_not_cover_is_refused(ev, ops):
    N, LIM, bank, pol, _, noise = mlp_scenario(ev, DEV)
    wide = ev.PeakAndStopPredictor(hidden_dim=48, device=DEV, seed=1)
    for kw in ({"fused": True}, {"fused": False}):
        with pytest.raises(RuntimeError, match=r"peak_stop_device=True.*hidden 48"):
            ev.evaluate(pol, mlp_env(bank, N), peak_stop=wide, max_steps=LIM, peak_stop_device=True, **kw)
    with pytest.raises(RuntimeError, match=r"window_size_v21 = 33"):
        ev.evaluate(pol, mlp_env(bank, N), peak_stop=make_predictor(ev, DEV), window_size_v21=33, max_steps=LIM, peak_stop_device=True)
    with pytest.raises(RuntimeError, match=r"uav_peak_stop_param_count.*hidden=48"):
        ops.peak_stop_scan(torch.zeros(10, device=DEV), 48, 20, torch.zeros(4, 5, device=DEV), torch.zeros(4, 19, device=DEV),
                           torch.zeros(4, dtype=torch.int32, device=DEV))
