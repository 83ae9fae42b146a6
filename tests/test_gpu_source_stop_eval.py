"""The estimator's stop rule through the public interface: evaluate(source_stop=...) and VecPPOTrainer(eval_source_stop=...) in the
set-up of tests/test_gpu_source_fit_eval.py, for the reasons given there: 64 envs x 64 steps over a two-field bank with sources near
(40, 40), a success radius of 2 cells, a turbulence channel of 5 .. 9, fresh LSTM h = 64, MLP and two-layer (tail route)
policies.  The kernel itself is tested in tests/test_gpu_source_stop.py."""
import numpy as np
import pytest
import torch

from _source_stop_cases import margins
from test_gpu_source_fit_eval import CHUNK, DEV, N, RADIUS, STEPS, bank, bits64, greedy_records, make_env, make_policy, make_trainer  # noqa: F401

pytestmark = pytest.mark.gpu
NEVER = {"patience": 1 << 30}


@pytest.fixture(scope="module")
def sf():
    from uavppo import source_fit
    return source_fit


@pytest.fixture(scope="module")
def ss():
    from uavppo import source_stop
    return source_stop


def check_against_statement(sf, ss, m, chunks, src, fit_kw=None, stop_kw=None, need=N // 4):
    """evaluate(source_stop=...)'s metrics against source_stop.stop_records on the records a plain GreedyRun leaves: up to an env's
    stop they are the records the evaluation saw, and behind it the statement reads none.  The records' margins are asserted first
    (a condition on the inputs: tests/_source_stop_cases.margins)."""
    fit_cfg, stop_cfg = sf.check_source_fit(**(fit_kw or {})), ss.check_source_stop(**(stop_kw or {}))
    ep = {key: np.concatenate([c[j] for c in chunks], 1) for j, key in enumerate(("flags", "obs", "pos"))}
    ep["ended"] = np.zeros(N, np.uint8)
    margins(sf, ss, ep, fit_kw or {}, stop_kw or {}, ([0] + list(np.cumsum([c[0].shape[1] for c in chunks])),))
    want = ss.stop_records(chunks, N, fit_cfg, stop_cfg)
    steps, state, pos_end = want["ep"]
    ended = (state & 1) != 0
    print(f"\nstopped by the rule {int(((state & 2) != 0).sum())} / {N}, by the env {int((ended & ((state & 2) == 0)).sum())}; stop steps "
          f"{np.percentile(want['stop_step'][want['stop_step'] > 0], [0, 50, 100]).tolist() if (want['stop_step'] > 0).any() else []}")
    assert ((state & 2) != 0).sum() >= need, "precondition: the set-up was chosen so that the rule ends episodes"
    assert np.array_equal(m["steps"], np.where(ended, steps, STEPS))
    assert np.array_equal(m["stopped_early"], (state & 2) != 0)
    assert np.array_equal(m["source_stop_step"], want["stop_step"]) and m["source_stop_step"].dtype == np.int64
    assert np.array_equal(m["steps"][m["stopped_early"]], m["source_stop_step"][m["stopped_early"]])
    dev = np.sqrt(((pos_end - src) ** 2).sum(1))
    assert np.allclose(m["deviations"][ended], dev[ended], rtol=1e-12, atol=0)
    from config import SUCCESS_DISTANCE_THRESHOLD
    assert np.array_equal(m["success"][ended], dev[ended] <= SUCCESS_DISTANCE_THRESHOLD)
    st, est, status = want["fit"]
    assert np.array_equal(m["source_status"], status)
    fit = status == 0
    assert np.abs(m["source_estimate"][fit] - est[fit, 0:2]).max() <= 1e-6
    # the estimate the rule stopped on is the estimate the estimator reports for the records up to the stop
    hit = want["stop_step"] > 0
    assert np.abs(m["source_estimate"][hit] - want["state"][hit, ss.EST:ss.EST + 2]).max() <= 1e-6
    return want


@pytest.mark.parametrize("kind", ["lstm", "mlp", "tail"])
def test_evaluate_source_stop_is_the_statement_on_its_records(bank, sf, ss, kind):
    from evaluate_with_lstm import evaluate
    pol = make_policy(kind)
    m = evaluate(pol, make_env(bank), max_steps=STEPS, chunk=CHUNK, source_stop=True)
    env = make_env(bank)
    chunks = greedy_records(pol, env, tail=kind == "tail")
    src = env.peek()[1].cpu().numpy().astype(np.float64)
    check_against_statement(sf, ss, m, chunks, src)
    fit = evaluate(pol, make_env(bank), max_steps=STEPS, chunk=CHUNK, source_fit=True)
    assert sorted(set(m) - set(fit)) == ["source_stop_step"]
    assert (m["steps"] <= fit["steps"]).all() and (m["steps"] < fit["steps"]).any()       # the rule ends episodes earlier, never later
    if kind == "lstm":                      # the keywords reach the kernel: both dicts, and another chunking decides the same
        kw, fkw = dict(settle_tol=2.0, patience=5, near=60.0, min_steps=12), dict(min_samples=6)
        m2 = evaluate(pol, make_env(bank), max_steps=STEPS, chunk=CHUNK, source_stop=kw, source_fit=fkw)
        check_against_statement(sf, ss, m2, chunks, src, fkw, kw, need=1)
        assert (m2["source_stop_step"][m2["source_stop_step"] > 0] >= 12).all()
        assert not np.array_equal(m2["source_stop_step"], m["source_stop_step"])
        m3 = evaluate(pol, make_env(bank), max_steps=STEPS, chunk=STEPS, source_stop=True)
        for key in ("steps", "stopped_early", "source_stop_step", "source_status"):
            assert np.array_equal(m3[key], m[key]), key


@pytest.mark.parametrize("kind", ["lstm", "mlp", "tail"])
def test_a_rule_that_cannot_fire_leaves_source_fits_metrics(bank, kind):
    from evaluate_with_lstm import evaluate
    pol = make_policy(kind)
    fit = evaluate(pol, make_env(bank), max_steps=STEPS, chunk=CHUNK, source_fit=True)
    m = evaluate(pol, make_env(bank), max_steps=STEPS, chunk=CHUNK, source_stop=NEVER)
    for key in fit:
        assert np.array_equal(fit[key], m[key], equal_nan=True) and fit[key].dtype == m[key].dtype, key
        if fit[key].dtype == np.float64:
            assert np.array_equal(bits64(fit[key]), bits64(m[key])), key
    assert not m["source_stop_step"].any() and not m["stopped_early"].any()


def test_evaluate_refuses_what_the_rule_cannot_follow(bank):
    from evaluate_with_lstm import PeakAndStopPredictor, evaluate
    pol, env = make_policy("lstm"), make_env(bank)
    with pytest.raises(ValueError, match="source_stop.*step-wise"):
        evaluate(pol, env, max_steps=8, fused=False, tail=False, source_stop=True)
    with pytest.raises(ValueError, match="source_stop.*step-wise"):
        evaluate(lambda obs: torch.zeros(obs.shape[0], 5, device=obs.device), env, max_steps=8, source_stop=True)
    with pytest.raises(ValueError, match="source_stop.*peak_stop"):
        evaluate(pol, env, max_steps=8, peak_stop=PeakAndStopPredictor(device=DEV, seed=1), source_stop=True)
    with pytest.raises(ValueError, match="source_stop.*controller"):
        evaluate(pol, env, max_steps=8, controller=object(), source_stop=True)
    with pytest.raises(ValueError, match="patience"):
        evaluate(pol, env, max_steps=8, source_stop={"patience": 0})
    with pytest.raises(ValueError, match="source_stop"):
        evaluate(pol, env, max_steps=8, source_stop="on")
    with pytest.raises(ValueError, match="min_samples"):
        evaluate(pol, env, max_steps=8, source_stop=True, source_fit={"min_samples": 2})


@pytest.mark.parametrize("kind", ["lstm", "mlp"])
def test_trainer_eval_source_stop(bank, sf, ss, kind):
    """Two iterations with eval_every=1: policy.flat and both Adam moments bit-identical with and without the rule; a curve row's
    source sums and stop count are those of a standalone run of the same evaluation."""
    from uavppo import eval_track as et
    ev = dict(eval_every=1, eval_envs=N, eval_max_steps=STEPS, eval_radius=RADIUS)
    on, off = make_trainer(bank, kind, eval_source_stop=True, **ev), make_trainer(bank, kind, **ev)
    flats = []
    for _ in range(2):
        for tr in (on, off):
            tr.train_iteration()
        flats.append(on.policy.flat.clone())
    same = lambda x, y: torch.equal(x.view(torch.int32), y.view(torch.int32))
    assert same(on.policy.flat, off.policy.flat) and same(on.exp_avg, off.exp_avg) and same(on.exp_avg_sq, off.exp_avg_sq)
    rows, rows_off = on.eval_tracker.curve(wait=True), off.eval_tracker.curve(wait=True)
    assert [r["iteration"] for r in rows] == [1, 2] and all("stopped" not in r and "source" not in r for r in rows_off)
    for r in rows:
        assert r["sums"][0] == N and r["source"].shape == (12,) and r["source"][0] == N and 0 <= r["stopped"] <= N
    print(f"\n[{kind}] stopped {[r['stopped'] for r in rows]} of {N}, fitted {[int(r['source'][1]) for r in rows]}, "
          f"mean steps {[float(r['sums'][2] / N) for r in rows]} against {[float(q['sums'][2] / N) for q in rows_off]} without the rule")
    assert rows[1]["stopped"] > 0 and rows[1]["sums"][2] < rows_off[1]["sums"][2]          # the rule ended episodes, earlier
    # a standalone run of evaluation 2: the policy as it saw it, the tracker's env arguments
    from uavppo import ops
    from uavppo.greedy import GreedyRun, policy_core
    from uavppo.vec_env import VecMethaneEnv
    t = on.eval_tracker
    on.policy.flat.copy_(flats[1])
    env = VecMethaneEnv(**t.env_args)
    env.current_radius = RADIUS
    env.reset()
    src = env.peek()[1].to(torch.float64).contiguous()
    k2, core = policy_core(on.policy)
    run, fit, stop = GreedyRun(k2, core, env), sf.SourceFit(N, DEV), ss.SourceStop(N, DEV)
    state = [torch.from_numpy(a).to(DEV) for a in et.fresh_episodes(N)]
    for t0 in range(0, STEPS, t.chunk):
        recs = run.chunk(t0, min(t.chunk, STEPS - t0))
        stop.scan(recs, t0, state[1], run.active)
        fit.chunk(recs, state[1])
        ops.greedy_reduce(recs, t0, *state)
    sums = fit.finish(src, float("nan"), float("nan")).cpu().numpy()
    assert np.array_equal(bits64(sums), bits64(rows[1]["source"]))
    assert rows[1]["stopped"] == float(((state[1] & 2) != 0).sum().item())
    assert rows[1]["stopped"] == float((stop.stop_steps() > 0).sum().item())
    # the curve file: Stop_Rate behind the six source columns, only with the option
    line = et.curve_row(rows[1]["iteration"], rows[1]["sums"], rows[1]["state"], rows[1]["source"], rows[1]["stopped"])
    assert len(line) == len(et.curve_columns(True, True)) == len(et.CURVE_COLUMNS) + 7 and et.curve_columns(True, True)[-1] == "Stop_Rate"
    assert line[-1] == rows[1]["stopped"] / N and et.curve_columns(True) == et.curve_columns(True, False)
    assert et.curve_columns(False, False) == et.CURVE_COLUMNS


def test_tracker_run_with_the_rule_reads_nothing_on_the_host(bank):
    tr = make_trainer(bank, "lstm", eval_every=1, eval_envs=N, eval_max_steps=STEPS, eval_radius=RADIUS, eval_source_stop=True)
    tr.train_iteration()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        tr.eval_tracker.run(2)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    rows = tr.eval_tracker.curve(wait=True)
    assert [r["iteration"] for r in rows] == [1, 2] and rows[1]["source"][0] == N and "stopped" in rows[1]


def test_trainer_refuses_a_bad_option_before_the_device(bank):
    with pytest.raises(ValueError, match="settle_tol"):
        make_trainer(bank, "lstm", eval_source_stop={"settle_tol": -1.0})
    with pytest.raises(ValueError, match="source_stop"):
        make_trainer(bank, "lstm", eval_every=1, eval_source_stop=3)
