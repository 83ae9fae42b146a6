"""The in-training greedy evaluation (VecPPOTrainer(eval_every=...), uavppo/eval_track.py) on a trainer of 32 envs x 16 steps with
64 evaluation envs, eval_max_steps=48 and eval_chunk=16: parity with evaluate(), repeatability, that training is untouched to the
bit (also under the forced one-rank collective path), the best model, and the scripts' files.

Deviation bar: EvalTracker forms sqrt(dx * dx + dy * dy) in f64 without contraction; evaluate() calls torch.linalg.norm on the
device.  The bar started at 4 * 2^-52 relative (room for a fused multiply-add inside torch's reduction); the maximum measured on
an MI355X was 0 on all three routes, so the bar is equality of the bits.  The figure is printed before it is
asserted."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "uav-wrf-les-ppo-lstm_amd")
N_ENV, T = 32, 16
EVAL = dict(eval_envs=64, eval_max_steps=48, eval_chunk=16)
ROUTES = {"fused_lstm": (dict(policy="lstm", hidden=64), "fused"), "fused_mlp": (dict(policy="mlp"), "fused"),
          "tail": (dict(policy="lstm", hidden=64, layers=2), "tail")}


def bits(t):
    t = t.detach().contiguous()
    return t.view({4: torch.int32, 8: torch.int64, 1: torch.uint8}[t.element_size()])


def same(a, b):
    return torch.equal(bits(a), bits(b))


def same64(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=np.float64).view(np.uint64), np.ascontiguousarray(b, dtype=np.float64).view(np.uint64))


def make(route, seed=11, **kw):
    from uavppo.trainer import VecPPOTrainer
    return VecPPOTrainer(N_ENV, T, device=DEV, seed=seed, **ROUTES[route][0], **kw)


def same_training(a, b):
    return (same(a.policy.flat, b.policy.flat) and same(a.exp_avg, b.exp_avg) and same(a.exp_avg_sq, b.exp_avg_sq)
            and same(a.env_state, b.env_state) and a.opt_step == b.opt_step)


def test_the_option_is_off_by_default():
    tr = make("fused_lstm")
    assert tr.eval_tracker is None and tr.eval["eval_every"] is None
    tr.train_iteration()
    tr.evaluate_if_due()                                    # nothing to do


@pytest.mark.parametrize("route", list(ROUTES))
def test_parity_with_evaluate_and_repeatability(route):
    from evaluate_with_lstm import evaluate
    from uavppo.vec_env import VecMethaneEnv
    tr = make(route, eval_every=1, **EVAL)
    t = tr.eval_tracker
    assert t.route == ROUTES[route][1] and t.limit == 48 and t.chunk == 16 and t.N == 64
    for _ in range(2):                                      # parameters that have moved off the initialisation
        tr.collect()
        tr.update()
    flat0 = tr.policy.flat.clone()
    t.run(1)
    torch.cuda.synchronize()
    got = {"steps": t.steps.cpu().numpy(), "success": t.success.cpu().numpy() != 0, "deviation": t.deviation.cpu().numpy()}
    m = evaluate(tr.policy, VecMethaneEnv(**t.env_args), max_steps=48)
    near = np.abs(m["deviations"] - 40.0).min()
    assert near > 1e-6, f"precondition: a yardstick deviation lies {near:g} from success_distance"
    rel = np.abs(got["deviation"] - m["deviations"]) / np.abs(m["deviations"])
    print(f"\n[{route}] max relative deviation difference against evaluate(): {rel.max():.3e}; successes {int(got['success'].sum())} / 64; "
          f"steps {got['steps'].min()} .. {got['steps'].max()}")
    assert np.array_equal(got["steps"], m["steps"]) and np.array_equal(got["success"], m["success"])
    assert same64(got["deviation"], m["deviations"]), rel.max()
    # the sums are the numpy definition's over the per-env values, and a second evaluation of unchanged parameters repeats them
    t.run(2)
    rows = t.curve(wait=True)
    assert [r["iteration"] for r in rows] == [1, 2] and same64(rows[0]["sums"], rows[1]["sums"])
    S = rows[0]["sums"]
    assert S[0] == 64 and S[1] == got["success"].sum() and S[2] == got["steps"].sum() and S[7] == 0
    assert S[6] == (t.ep_state.cpu().numpy() & 1 == 0).sum()
    assert rows[0]["state"][6] == 1.0 and rows[1]["state"][6] == 0.0 and rows[1]["state"][3] == 2.0       # a tie keeps the earlier
    assert same(tr.policy.flat, flat0) and same(t.best_flat(), flat0)


@pytest.mark.parametrize("route", list(ROUTES))
def test_training_is_untouched(route):
    a, b = make(route, eval_every=2, **EVAL), make(route)
    for _ in range(4):
        a.train_iteration()
        b.train_iteration()
    assert same_training(a, b)
    if a.kind == "lstm":
        assert same(a._state, b._state)
    rows = a.eval_tracker.curve(wait=True)
    assert [r["iteration"] for r in rows] == [2, 4] and all(r["sums"][0] == 64 for r in rows)
    a.losses()


_CHILD = """
import json, sys
sys.path[:0] = [%r, %r]
import torch
from uavppo.dist_utils import collectives_on, use_abi_collectives
from uavppo.trainer import VecPPOTrainer
use_abi_collectives(0, 1, "cuda:0")
assert collectives_on()
kw = dict(policy="lstm", hidden=64, device="cuda:0", seed=11)
a = VecPPOTrainer(32, 16, eval_every=2, eval_envs=64, eval_max_steps=48, eval_chunk=16, **kw)
b = VecPPOTrainer(32, 16, **kw)
assert a.eval_tracker.collectives
for _ in range(4):
    a.train_iteration()
    b.train_iteration()
eq = lambda x, y: bool(torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8)))
same = all(eq(getattr(a, n), getattr(b, n)) for n in ("exp_avg", "exp_avg_sq", "env_state")) and eq(a.policy.flat, b.policy.flat) and a.opt_step == b.opt_step
rows = a.eval_tracker.curve(wait=True)
a.losses()
print(json.dumps({"same": same, "rows": [[r["iteration"], r["sums"].view("uint64").tolist(), r["state"].view("uint64").tolist()] for r in rows]}))
"""


def test_training_is_untouched_under_forced_one_rank_collectives():
    """The eight sums' all-reduce issued for real on a one-rank RCCL communicator (process-wide state, hence a child process): the
    trainer with the evaluation equals the one without, and the curve equals the one computed without collectives."""
    r = subprocess.run([sys.executable, "-c", _CHILD % (ROOT, PKG)], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, UAVPPO_FORCE_COLLECTIVES="1"))
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["same"]
    tr = make("fused_lstm", eval_every=2, **EVAL)
    for _ in range(4):
        tr.train_iteration()
    rows = tr.eval_tracker.curve(wait=True)
    assert out["rows"] == [[r["iteration"], r["sums"].view(np.uint64).tolist(), r["state"].view(np.uint64).tolist()] for r in rows]


@pytest.mark.parametrize("route", ["fused_lstm", "fused_mlp"])
def test_best_model_is_the_one_better_rule_picks(route, tmp_path):
    from uavppo import eval_track as et
    tr = make(route, eval_every=1, lr=1e-3, **EVAL)
    t = tr.eval_tracker
    kept = []
    for i in range(6):
        tr.train_iteration()
        kept.append(tr.policy.flat.clone())                 # what evaluation i + 1 saw
        if i == 0:
            assert same(t.best_flat(), kept[0])             # the first valid row is always better
    rows = t.curve(wait=True)
    assert [r["iteration"] for r in rows] == [1, 2, 3, 4, 5, 6]
    state, pick, took = np.zeros(et.BEST_N), None, []
    for i, r in enumerate(rows):
        state = et.better_rule(state, r["sums"], r["iteration"])
        assert same64(state, r["state"]), i                 # the device decided what the numpy rule decides
        took.append(int(state[6]))
        pick = i if state[6] == 1.0 else pick
    print(f"\n[{route}] successes {[int(r['sums'][1]) for r in rows]} steps {[int(r['sums'][2]) for r in rows]} took {took}")
    assert pick is not None and state[2] == pick + 1
    assert same(t.best_flat(), kept[pick])
    sd = t.best_state_dict()
    assert sorted(sd) == sorted(tr.policy.state_dict())
    tr.policy.flat.copy_(kept[pick])
    assert all(same(sd[k], v) for k, v in tr.policy.state_dict().items())
    et.write_curve(str(tmp_path / "c.csv"), rows)
    lines = open(tmp_path / "c.csv").read().splitlines()
    assert lines[0].split(",") == et.CURVE_COLUMNS and [int(ln.split(",")[-1]) for ln in lines[1:]] == took


def _script(name, file, monkeypatch, **cfg):
    """A training script loaded with config names set for the duration of the test (the scripts import them by name)."""
    import importlib.util
    import config
    for k, v in cfg.items():
        assert hasattr(config, k), k
        monkeypatch.setattr(config, k, v)
    spec = importlib.util.spec_from_file_location(name, os.path.join(PKG, file))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


CFG = dict(NUM_ENVS=32, HORIZON=16, POLICY="lstm", HIDDEN=64, EPOCHS=3)


def test_train_script_writes_the_curve_and_the_best_model(tmp_path, monkeypatch):
    from evaluate_with_lstm import load_lstm_policy
    from uavppo import eval_track as et
    run = lambda d, m: m.train_ppo_vectorised(iterations=3, csv_path=str(tmp_path / d / "episodes.csv"),
                                              model_path=str(tmp_path / d / "model.pth"), log_every=0)
    for d in ("on", "off", "off2"):
        os.makedirs(tmp_path / d)
    m = _script("train_ppo2_0_eval", "train_ppo2.0.py", monkeypatch, EVAL_EVERY=1, EVAL_ENVS=64, EVAL_MAX_STEPS=48, **CFG)
    tr, _ = run("on", m)
    lines = open(tmp_path / "on" / et.CURVE_FILE).read().splitlines()
    assert lines[0].split(",") == et.CURVE_COLUMNS and [ln.split(",")[0] for ln in lines[1:]] == ["1", "2", "3"]
    assert all(ln.split(",")[1] == "64" for ln in lines[1:])
    rows = tr.eval_tracker.curve()
    assert [int(ln.split(",")[-1]) for ln in lines[1:]] == [int(r["state"][6]) for r in rows] and lines[1].endswith(",1")
    pol = load_lstm_policy(str(tmp_path / "on" / et.BEST_MODEL_FILE), DEV)
    assert same(pol.flat, tr.eval_tracker.best_flat())
    assert sorted(torch.load(tmp_path / "on" / et.BEST_MODEL_FILE)) == sorted(torch.load(tmp_path / "on" / "model.pth"))
    # without the option: no new file, and outputs that the evaluation of the run above did not change by a byte
    m = _script("train_ppo2_0_plain", "train_ppo2.0.py", monkeypatch, EVAL_EVERY=None, **CFG)
    run("off", m)
    run("off2", m)
    read = lambda d, f: open(tmp_path / d / f, "rb").read()
    assert sorted(os.listdir(tmp_path / "off")) == ["episodes.csv", "model.pth"]
    assert read("off", "episodes.csv") == read("off2", "episodes.csv") and read("off", "model.pth") == read("off2", "model.pth")
    assert read("on", "episodes.csv") == read("off", "episodes.csv") and read("on", "model.pth") == read("off", "model.pth")


def test_gail_script_writes_the_curve_and_the_best_model(tmp_path, monkeypatch):
    from uavppo import eval_track as et
    rng = np.random.RandomState(3)
    np.savez(str(tmp_path / "expert_data.npz"), states=rng.rand(64, 6).astype(np.float32), actions=rng.randint(0, 5, 64).astype(np.int64))
    m = _script("train_ppo_gail_eval", "train_ppo_gail.py", monkeypatch, EPOCHS=2, EVAL_EVERY=2, EVAL_ENVS=64, EVAL_MAX_STEPS=48)
    tr = m.train_ppo_gail(num_episodes=10 ** 6, num_envs=32, horizon=16, expert_path=str(tmp_path / "expert_data.npz"), policy="mlp",
                          max_iterations=4, model_path=str(tmp_path / "g.pth"), disc_path=str(tmp_path / "d.pth"))
    lines = open(tmp_path / et.CURVE_FILE).read().splitlines()
    assert [ln.split(",")[0] for ln in lines[1:]] == ["2", "4"] and lines[1].endswith(",1")
    sd = torch.load(tmp_path / et.BEST_MODEL_FILE)
    assert sorted(sd) == sorted(tr.policy.state_dict())
    best = tr.eval_tracker.best_state_dict()
    assert all(same(sd[k].to(DEV), best[k]) for k in sd)
