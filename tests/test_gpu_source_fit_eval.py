"""The source estimate through the public interface: evaluate(source_fit=...), ModelEvaluator.run_evaluation(source_fit=...) and
VecPPOTrainer(eval_source_fit=...) on 64 envs x 64 steps over a two-field materialised bank built here in numpy, whose sources
stand near (40, 40): the envs start at the origin, so a fresh policy's records are usable from the first step.  Two more choices
keep a fresh policy's track fit for a fit: a success radius of 2 cells (at the default 50 the first step from the origin already
ends the episode, which leaves one record), and a turbulence channel of 5 .. 9 (the wind's displacement grows with it, so a policy
that repeats one action still leaves a track that is not a straight line).  The policy seeds are ones whose greedy action moves.
The kernels themselves are tested in tests/test_gpu_source_fit.py."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, STEPS, CHUNK = 64, 64, 16
SIGMA = 500.0 / 16.0
RADIUS = 2.0
SEEDS = {"lstm": 3, "mlp": 1, "tail": 2}
SOURCES = np.array([[40.0, 40.0], [44.0, 37.0]])
POLICIES = ["lstm", "mlp"]


@pytest.fixture(scope="module")
def bank():
    """(bank f64 [2, 500, 500, 2] of (conc, tke), sources f64 [2, 2]): E3's formula on every cell"""
    rng = np.random.default_rng(5)
    x, y = np.meshgrid(np.arange(500.0), np.arange(500.0), indexing="ij")
    out = np.empty((2, 500, 500, 2))
    for f, (sx, sy) in enumerate(SOURCES):
        tke = rng.uniform(5.0, 9.0, (500, 500))
        d2 = (x - sx) ** 2 + (y - sy) ** 2
        out[f, :, :, 0] = np.clip(100.0 * np.exp(-d2 / (2.0 * SIGMA ** 2)) + tke, 0.0, 100.0)
        out[f, :, :, 1] = tke
    return out, SOURCES.copy()


@pytest.fixture(scope="module")
def sf():
    from uavppo import source_fit
    return source_fit


def make_env(bank, n=N, seed=3):
    from uavppo.vec_env import VecMethaneEnv
    env = VecMethaneEnv(n, "v2.0", DEV, seed=seed, bank=bank[0], bank_sources=bank[1])
    env.current_radius = RADIUS
    return env


def make_policy(kind):
    from uavppo.policy import LSTMActorCritic, MLPActorCritic
    if kind == "tail":                                          # two layers: the fused kernel refuses, the tail route takes it
        return LSTMActorCritic(6, 64, 2, device=DEV, seed=SEEDS[kind])
    return LSTMActorCritic(6, 64, 1, device=DEV, seed=SEEDS[kind]) if kind == "lstm" else MLPActorCritic(6, 5, device=DEV, seed=SEEDS[kind])


def bits64(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def greedy_records(policy, env, rule=None, tail=False):
    """The records evaluate() reads, chunk by chunk, as numpy: [(flags, obs, pos)]"""
    from uavppo.greedy import GreedyRun, policy_core
    kind, core = policy_core(policy)
    env.reset()
    run = GreedyRun(kind, core, env, rule, tail=tail)
    out = []
    for t0 in range(0, STEPS, CHUNK):
        recs = run.chunk(t0, CHUNK)
        out.append(tuple(recs[k].cpu().numpy().copy() for k in ("flags", "obs", "pos")))
    return out


def check_against_statement(sf, m, chunks, src, cfg=None, need=N // 2):
    """Statuses equal where the statement's |a3| is not within 1e-9 of 0; estimates agree to 1e-6 cells"""
    st, est, status = sf.fit_records(chunks, N, **(cfg or {}))
    a, _ = sf.coefficients(st, sf.check_source_fit(**(cfg or {}))["min_pivot"])
    with np.errstate(invalid="ignore"):
        sure = ~(np.abs(a[:, 3]) <= 1e-9)
    assert np.array_equal(m["source_status"][sure], status[sure]) and m["source_status"].dtype == np.uint8
    fit = sure & (status == 0)
    print(f"\nfitted {int(fit.sum())} / {N}; statuses {np.bincount(status, minlength=4).tolist()}; "
          f"median error {np.median(m['source_error'][fit]) if fit.any() else float('nan'):.3g} cells")
    assert fit.sum() >= need, "precondition: the bank was built so that most episodes can be fitted"
    assert np.abs(m["source_estimate"][fit] - est[fit, 0:2]).max() <= 1e-6
    assert np.allclose(m["source_sigma"][fit], est[fit, 2], rtol=1e-9, atol=0)
    assert np.allclose(m["source_peak"][fit], est[fit, 3], rtol=1e-9, atol=0)
    assert np.allclose(m["source_strength"][fit], est[fit, 4], rtol=1e-9, atol=0)
    assert np.array_equal(bits64(m["source_max_sample"][sure]), bits64(est[sure, 5:8]))
    err = np.sqrt(((est[:, 0:2] - src) ** 2).sum(1))
    assert np.abs(m["source_error"][fit] - err[fit]).max() <= 2e-6 and np.isnan(m["source_error"][sure & (status != 0)]).all()
    assert m["source_estimate"].shape == (N, 2) and m["source_max_sample"].shape == (N, 3)
    return st, est, status


@pytest.mark.parametrize("kind", POLICIES)
def test_evaluate_source_fit_is_the_statement_on_its_records(bank, sf, kind):
    from evaluate_with_lstm import evaluate
    pol = make_policy(kind)
    plain = evaluate(pol, make_env(bank), max_steps=STEPS, chunk=CHUNK)
    m = evaluate(pol, make_env(bank), max_steps=STEPS, chunk=CHUNK, source_fit=True)
    for key in plain:                                           # the other metric arrays: exactly those of source_fit=None
        assert np.array_equal(plain[key], m[key]) and plain[key].dtype == m[key].dtype, key
    assert sorted(set(m) - set(plain)) == ["source_error", "source_estimate", "source_max_sample", "source_peak", "source_sigma",
                                           "source_status", "source_strength"]
    env = make_env(bank)
    chunks = greedy_records(pol, env)
    src = env.peek()[1].cpu().numpy().astype(np.float64)
    check_against_statement(sf, m, chunks, src)
    # exact plumes: the estimate is the source.  The median within the 1e-3 cells of tests/test_source_fit_host.py; the largest is
    # printed, not bounded: how well a near-straight track conditions the fit is the policy's doing
    fit = m["source_status"] == 0
    print(f"source error median {np.median(m['source_error'][fit]):.3g} max {m['source_error'][fit].max():.3g} cells")
    assert np.median(m["source_error"][fit]) <= 1e-3
    # a dict of keywords reaches the kernels
    cfg = dict(use_tke=False, background=7.0, floor=20.0, min_samples=4)
    m2 = evaluate(pol, make_env(bank), max_steps=STEPS, chunk=CHUNK, source_fit=cfg)
    check_against_statement(sf, m2, chunks, src, cfg, need=0)
    assert not np.array_equal(m2["source_status"], m["source_status"]) or not np.array_equal(bits64(m2["source_estimate"]), bits64(m["source_estimate"]))


def test_evaluate_refuses_what_the_estimator_cannot_follow(bank):
    from evaluate_with_lstm import PeakAndStopPredictor, evaluate
    pol, env = make_policy("lstm"), make_env(bank)
    with pytest.raises(ValueError, match="step-wise"):
        evaluate(pol, env, max_steps=8, fused=False, tail=False, source_fit=True)
    with pytest.raises(ValueError, match="step-wise"):
        evaluate(lambda obs: torch.zeros(obs.shape[0], 5, device=obs.device), env, max_steps=8, source_fit=True)
    with pytest.raises(ValueError, match="peak_stop"):
        evaluate(pol, env, max_steps=8, peak_stop=PeakAndStopPredictor(device=DEV, seed=1), source_fit=True)
    with pytest.raises(ValueError, match="controller"):
        evaluate(pol, env, max_steps=8, controller=object(), source_fit=True)
    with pytest.raises(ValueError, match="min_samples"):
        evaluate(pol, env, max_steps=8, source_fit={"min_samples": 2})
    with pytest.raises(ValueError, match="source_fit"):
        evaluate(pol, env, max_steps=8, source_fit="on")


def test_evaluate_on_the_tail_route(bank, sf):
    from evaluate_with_lstm import evaluate
    from uavppo.greedy import policy_route
    pol = make_policy("tail")
    assert policy_route(pol, make_env(bank), who="test") == "tail"
    m = evaluate(pol, make_env(bank), max_steps=STEPS, chunk=CHUNK, source_fit=True)
    f = evaluate(pol, make_env(bank), max_steps=STEPS, chunk=CHUNK)
    assert all(np.array_equal(f[k], m[k]) for k in f)
    env = make_env(bank)
    chunks = greedy_records(pol, env, tail=True)
    check_against_statement(sf, m, chunks, env.peek()[1].cpu().numpy().astype(np.float64))


def test_model_evaluator_writes_source_estimates(bank, sf, tmp_path):
    """The stop rule's bit3 ends an episode for the estimator; evaluation_results.csv stays byte for byte."""
    from evaluate_model import ModelEvaluator
    pol = make_policy("lstm")
    os.makedirs(tmp_path / "a")
    os.makedirs(tmp_path / "b")
    a = ModelEvaluator(pol, N, DEV, env=make_env(bank)).run_evaluation(max_steps=STEPS, chunk=CHUNK, csv_path=str(tmp_path / "a" / "evaluation_results.csv"))
    ev = ModelEvaluator(pol, N, DEV, env=make_env(bank))
    b = ev.run_evaluation(max_steps=STEPS, chunk=CHUNK, csv_path=str(tmp_path / "b" / "evaluation_results.csv"), source_fit=True)
    assert sorted(os.listdir(tmp_path / "a")) == ["evaluation_results.csv"]
    assert sorted(os.listdir(tmp_path / "b")) == ["evaluation_results.csv", sf.ESTIMATE_FILE]
    assert open(tmp_path / "a" / "evaluation_results.csv", "rb").read() == open(tmp_path / "b" / "evaluation_results.csv", "rb").read()
    assert all(np.array_equal(a[k], b[k]) for k in a)
    env = make_env(bank)
    chunks = greedy_records(pol, env, ev._rule())
    check_against_statement(sf, b, chunks, env.peek()[1].cpu().numpy().astype(np.float64))
    lines = open(tmp_path / "b" / sf.ESTIMATE_FILE).read().splitlines()
    assert lines[0].split(",") == sf.ESTIMATE_COLUMNS and len(lines) == N + 1
    first = lines[1].split(",")
    assert first[0] == "1" and first[1] in ("fitted", "few", "degenerate", "not_a_peak")
    with pytest.raises(ValueError, match="step-wise"):
        ev.run_evaluation(max_steps=8, fused=False, tail=False, csv_path=None, source_fit=True)


def make_trainer(bank, kind, **kw):
    from uavppo.trainer import VecPPOTrainer
    pol = dict(policy="lstm", hidden=64) if kind == "lstm" else dict(policy="mlp")
    return VecPPOTrainer(32, 16, device=DEV, seed=11, variant="v2.0", bank=bank[0], bank_sources=bank[1], **pol, **kw)


@pytest.mark.parametrize("kind", POLICIES)
def test_trainer_eval_source_fit(bank, sf, kind):
    """Two iterations with eval_every=1: policy.flat bit-identical to the run without the estimate (and to the run without any
    evaluation), the bookkeeping's rows unchanged, and the rows' "source" the sums a standalone SourceFit gives."""
    from uavppo import eval_track as et
    ev = dict(eval_every=1, eval_envs=N, eval_max_steps=STEPS, eval_radius=RADIUS)
    on, off, none = make_trainer(bank, kind, eval_source_fit=True, **ev), make_trainer(bank, kind, **ev), make_trainer(bank, kind)
    flats = []
    for _ in range(2):
        for tr in (on, off, none):
            tr.train_iteration()
        flats.append(on.policy.flat.clone())
    same = lambda x, y: torch.equal(x.view(torch.int32), y.view(torch.int32))
    assert same(on.policy.flat, off.policy.flat) and same(on.policy.flat, none.policy.flat)
    assert same(on.exp_avg, off.exp_avg) and same(on.exp_avg_sq, off.exp_avg_sq)
    assert same(on.eval_tracker.best_flat(), off.eval_tracker.best_flat())
    rows, rows_off = on.eval_tracker.curve(wait=True), off.eval_tracker.curve(wait=True)
    assert [r["iteration"] for r in rows] == [1, 2] and all("source" not in r for r in rows_off)
    for r, q in zip(rows, rows_off):
        assert np.array_equal(bits64(r["sums"]), bits64(q["sums"])) and np.array_equal(bits64(r["state"]), bits64(q["state"]))
        assert r["source"].shape == (12,) and r["source"][0] == N and r["source"][1:5].sum() == N
        assert r["source"][8] == 0.0 and r["source"][9] == 0.0                 # a user bank: the plume's width is not known
    print(f"\n[{kind}] fitted {[int(r['source'][1]) for r in rows]} of {N}; mean error "
          f"{[float(r['source'][5] / r['source'][1]) if r['source'][1] else float('nan') for r in rows]}")
    # a standalone SourceFit over the same evaluation: the policy as evaluation 2 saw it, the tracker's env arguments
    from uavppo.greedy import GreedyRun, policy_core
    from uavppo.vec_env import VecMethaneEnv
    t = on.eval_tracker
    on.policy.flat.copy_(flats[1])
    env = VecMethaneEnv(**t.env_args)
    env.current_radius = RADIUS
    env.reset()
    src = env.peek()[1].to(torch.float64).contiguous()
    k2, core = policy_core(on.policy)
    run, fit = GreedyRun(k2, core, env), sf.SourceFit(N, DEV)
    state = [torch.from_numpy(a).to(DEV) for a in et.fresh_episodes(N)]
    from uavppo import ops
    for t0 in range(0, STEPS, t.chunk):
        recs = run.chunk(t0, min(t.chunk, STEPS - t0))
        fit.chunk(recs, state[1])
        ops.greedy_reduce(recs, t0, *state)
    sums = fit.finish(src, float("nan"), float("nan")).cpu().numpy()
    assert np.array_equal(bits64(sums), bits64(rows[1]["source"]))
    # the curve file: six more columns, only with the option
    line = et.curve_row(rows[1]["iteration"], rows[1]["sums"], rows[1]["state"], rows[1]["source"])
    assert len(line) == len(et.curve_columns(True)) == len(et.CURVE_COLUMNS) + 6 and et.curve_columns(False) == et.CURVE_COLUMNS
    assert line[len(et.CURVE_COLUMNS)] == rows[1]["source"][1] / N


def test_tracker_run_reads_nothing_on_the_host(bank):
    tr = make_trainer(bank, "lstm", eval_every=1, eval_envs=N, eval_max_steps=STEPS, eval_radius=RADIUS, eval_source_fit=True)
    tr.train_iteration()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        tr.eval_tracker.run(2)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    rows = tr.eval_tracker.curve(wait=True)
    assert [r["iteration"] for r in rows] == [1, 2] and rows[1]["source"][0] == N


def test_trainer_refuses_a_bad_option_before_the_device(bank):
    with pytest.raises(ValueError, match="floor"):
        make_trainer(bank, "lstm", eval_source_fit={"floor": -1.0})
    with pytest.raises(ValueError, match="source_fit"):
        make_trainer(bank, "lstm", eval_every=1, eval_source_fit=3)
