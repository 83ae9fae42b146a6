"""Learning-rate and entropy schedules on the GPU: uav_clip_adam_dlr against uav_clip_adam, uav_lr_adapt / uav_lr_init against
the numpy rule of uavppo/lr_control.py, and the three modes of VecPPOTrainer's lr_schedule through whole iterations.  -m gpu.

Bars.  Every comparison here is bit for bit: the device-rate Adam step forms the host's expression on the host's operands, the
adapt kernel runs adapt_rule's f64 operations in its order, and a schedule that hands a kernel the same float hands it the
same work."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from _lr_control_cases import D, F, HI, LO, TABLE, random_rows

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ops():
    from uavppo import ops as o
    return o


def bits(t):
    return t.detach().contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def same(a, b):
    return torch.equal(bits(a), bits(b))


def same64(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=np.float64).view(np.uint64), np.ascontiguousarray(b, dtype=np.float64).view(np.uint64))


def same_optimiser(a, b):
    return same(a.policy.flat, b.policy.flat) and same(a.exp_avg, b.exp_avg) and same(a.exp_avg_sq, b.exp_avg_sq) and a.opt_step == b.opt_step


# ------------------------------------------------------------------------------------------------ 1: the device-rate Adam step
def _adam_pair(ops, p, g, m, v, step, lr, max_norm):
    """(outputs of clip_adam with lr = lr_dev[0], outputs of clip_adam_dlr) on clones of the same inputs."""
    lr_dev = torch.tensor([lr], dtype=torch.float32, device=DEV)
    out = []
    for dlr in (False, True):
        pp, mm, vv = p.clone(), m.clone(), v.clone()
        gn, pm = (torch.full((1,), -1.0, dtype=torch.float32, device=DEV) for _ in range(2))
        if dlr:
            ops.clip_adam_dlr(pp, g, mm, vv, step, lr_dev, max_norm=max_norm, gnorm_out=gn, pmax_out=pm)
        else:
            ops.clip_adam(pp, g, mm, vv, step, float(lr_dev.item()), max_norm=max_norm, gnorm_out=gn, pmax_out=pm)
        out.append((pp, mm, vv, gn, pm))
    return out


@pytest.mark.parametrize("n", [1, 255, 256, 257, 36230, 1024 * 256 + 3])       # the last: past the 256-block cap of the norm pass
def test_clip_adam_dlr_is_clip_adam_bit_for_bit(ops, n):
    gen = torch.Generator(device=DEV).manual_seed(n)
    p = torch.randn(n, generator=gen, device=DEV)
    g = torch.randn(n, generator=gen, device=DEV)
    m = torch.randn(n, generator=gen, device=DEV) * 0.1
    v = torch.rand(n, generator=gen, device=DEV) * 0.01
    g_above, g_below = g * (2.0 / g.norm()), g * (0.1 / g.norm())               # norm 2 (clipped at 0.5) and 0.1 (not clipped)
    cases = [(gg, step, lr, 0.5) for gg in (g_above, g_below) for step in (1, 2, 1000) for lr in (3e-5, 1e-2, 1e-6)]
    cases.append((g, 3, 3e-5, 0.0))                                             # clipping off
    g_nan = g_above.clone()
    g_nan[n // 2] = float("nan")
    cases.append((g_nan, 2, 3e-5, 0.5))                                         # a NaN: the same NaN pattern everywhere
    for gg, step, lr, max_norm in cases:
        want, got = _adam_pair(ops, p, gg, m, v, step, lr, max_norm)
        for name, a, b in zip(("param", "exp_avg", "exp_avg_sq", "gnorm_out", "pmax_out"), want, got):
            assert same(a, b), (name, n, step, lr, max_norm)
        assert not same(want[1], m)                                             # a step was taken
    assert torch.isnan(got[0]).all() and torch.isnan(got[3]).all() and torch.isinf(got[4]).all()      # (the NaN case, as uav_clip_adam documents)
    want, got = _adam_pair(ops, p, g_above, m, v, 1, 3e-5, 0.5)
    assert abs(got[3].item() - 2.0) < 1e-5


def test_clip_adam_dlr_reads_the_rate_on_the_stream(ops):
    """The rate a kernel wrote just before, never seen by the host: lr_init then the step, against clip_adam with that f32."""
    n = 1000
    gen = torch.Generator(device=DEV).manual_seed(5)
    p, g = torch.randn(n, generator=gen, device=DEV), torch.randn(n, generator=gen, device=DEV)
    m, v = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    state = torch.zeros(ops.LR_STATE_N, dtype=torch.float64, device=DEV)
    lr_dev = torch.zeros(1, dtype=torch.float32, device=DEV)
    pp, mm, vv = p.clone(), m.clone(), v.clone()
    ops.lr_init(state, 1.0 / 3.0 * 1e-3, lr_out=lr_dev)
    ops.clip_adam_dlr(pp, g, mm, vv, 1, lr_dev)
    ops.clip_adam(p, g, m, v, 1, float(np.float32(1.0 / 3.0 * 1e-3)))
    assert same(p, pp) and same(m, mm) and same(v, vv)


# ------------------------------------------------------------------------------------------------ 2: the rule as a kernel
def _adapt(ops, state, s8, desired, factor, lo, hi):
    st = torch.as_tensor(np.asarray(state, dtype=np.float64)).to(DEV)
    out = torch.full((1,), -1.0, dtype=torch.float32, device=DEV)
    ops.lr_adapt(st, torch.as_tensor(np.asarray(s8, dtype=np.float64)).to(DEV), desired, factor, lo, hi, lr_out=out)
    return st.cpu().numpy(), out.cpu().numpy()


def test_lr_init_and_the_table(ops):
    from uavppo.lr_control import adapt_rule, fresh_state
    for name, lr, s8, want_lr, slot in TABLE:
        st = torch.full((ops.LR_STATE_N,), 7.0, dtype=torch.float64, device=DEV)
        out = ops.lr_init(st, lr)
        assert same64(st.cpu().numpy(), fresh_state(lr)) and out.cpu().numpy().view(np.uint32)[0] == np.float32(lr).view(np.uint32), name
        got, lr_out = _adapt(ops, st.cpu().numpy(), s8, D, F, LO, HI)
        want = adapt_rule(fresh_state(lr), s8, D, F, LO, HI)
        assert same64(got, want), (name, got, want)
        assert got[0] == np.float64(want_lr) and got[ops.LR_STATE_NAMES.index(slot)] == 1.0, name
        assert lr_out.view(np.uint32)[0] == np.float32(want[0]).view(np.uint32), name


def test_forty_in_a_row_on_the_device(ops):
    st_up = torch.zeros(ops.LR_STATE_N, dtype=torch.float64, device=DEV)
    st_dn = torch.zeros(ops.LR_STATE_N, dtype=torch.float64, device=DEV)
    up, dn = ops.lr_init(st_up, 3e-5), ops.lr_init(st_dn, 3e-5)
    raise8, lower8 = (torch.as_tensor(TABLE[i][2]).to(DEV) for i in (1, 0))
    for _ in range(40):
        ops.lr_adapt(st_up, raise8, D, F, LO, HI, lr_out=up)
        ops.lr_adapt(st_dn, lower8, D, F, LO, HI, lr_out=dn)
    assert st_up.cpu().tolist() == [HI, 0.004 * 1024 / 1024, 40.0, 0.0, 0.0, 0.0] and up.item() == float(np.float32(HI))
    assert st_dn.cpu().tolist() == [LO, 0.021 * 1024 / 1024, 0.0, 40.0, 0.0, 0.0] and dn.item() == float(np.float32(LO))


def test_two_hundred_random_rows(ops):
    from uavppo.lr_control import adapt_rule
    seen = set()
    for i, (state, s8, desired, factor, lo, hi) in enumerate(random_rows(200)):
        got, lr_out = _adapt(ops, state, s8, desired, factor, lo, hi)
        want = adapt_rule(state, s8, desired, factor, lo, hi)
        assert same64(got, want), (i, got, want)
        assert lr_out.view(np.uint32)[0] == np.float32(want[0]).view(np.uint32), i
        seen.add(int(np.argmax(want[2:] - state[2:])))
    assert seen == {0, 1, 2, 3}                                                 # raised, lowered, held and skipped all occur


def test_every_refusal_returns_non_zero_with_a_message(ops):
    from uavppo._lib import lib
    h = ops.Context.get(torch.device(DEV)).handle
    st = torch.zeros(ops.LR_STATE_N, dtype=torch.float64, device=DEV)
    d8 = torch.zeros(8, dtype=torch.float64, device=DEV)
    out = torch.zeros(1, dtype=torch.float32, device=DEV)
    s, d, o = (C.c_void_p(t.data_ptr()) for t in (st, d8, out))
    stream = None                                                               # the null stream: nothing is launched here
    good = dict(state=s, diag8=d, desired_kl=0.01, factor=1.5, lr_min=1e-6, lr_max=1e-2, lr_out=o)
    nan = float("nan")
    bad = [dict(state=None), dict(diag8=None), dict(lr_out=None), dict(factor=1.0), dict(factor=0.5), dict(factor=nan), dict(lr_min=0.0),
           dict(lr_min=-1.0), dict(lr_min=nan), dict(lr_min=1e-2, lr_max=1e-3), dict(lr_max=nan), dict(desired_kl=0.0), dict(desired_kl=nan)]
    for kw in bad:
        a = dict(good, **kw)
        rc = lib().uav_lr_adapt(h, a["state"], a["diag8"], a["desired_kl"], a["factor"], a["lr_min"], a["lr_max"], a["lr_out"], stream)
        assert rc != 0 and b"uav_lr_adapt" in lib().uav_last_error(), kw
    assert lib().uav_lr_adapt(None, s, d, 0.01, 1.5, 1e-6, 1e-2, o, stream) != 0
    for args in ((None, s, 3e-5, o), (h, None, 3e-5, o), (h, s, 3e-5, None), (h, s, 0.0, o), (h, s, nan, o), (h, s, float("inf"), o)):
        assert lib().uav_lr_init(*args, stream) != 0 and b"uav_lr_init" in lib().uav_last_error(), args
    torch.cuda.synchronize()
    assert st.abs().sum().item() == 0.0 and out.item() == 0.0                   # a refused call launched nothing
    p = torch.ones(8, device=DEV)
    pp = C.c_void_p(p.data_ptr())
    assert lib().uav_clip_adam_dlr(h, pp, pp, pp, pp, 8, 1, None, 0.9, 0.999, 1e-8, 0.5, None, None, stream) != 0
    assert b"uav_clip_adam_dlr" in lib().uav_last_error()
    assert lib().uav_clip_adam_dlr(h, pp, pp, pp, pp, 8, 0, o, 0.9, 0.999, 1e-8, 0.5, None, None, stream) != 0
    with pytest.raises(RuntimeError):
        ops.lr_adapt(st, d8, 0.01, 1.0, 1e-6, 1e-2)
    with pytest.raises(RuntimeError):
        ops.lr_adapt(st, d8[:4].contiguous(), 0.01, 1.5, 1e-6, 1e-2)
    with pytest.raises(RuntimeError):
        ops.clip_adam_dlr(p, p, p, p, 1, torch.zeros(1, dtype=torch.float64, device=DEV))


# ------------------------------------------------------------------------------------------------ 3-7: the trainer
N_ENV, T = 64, 16
CONFIGS = {"lstm": dict(policy="lstm", hidden=64), "mlp": dict(policy="mlp"),
           "lstm_shuffle": dict(policy="lstm", hidden=64, num_minibatches=2, shuffle_envs=True),
           "lstm_obs_norm": dict(policy="lstm", hidden=64, normalise_obs=True),
           "mlp_rows": dict(policy="mlp", minibatch_rows=384), "mlp_layered": dict(policy="mlp")}


def make(config, seed=11, **kw):
    from uavppo.trainer import VecPPOTrainer
    tr = VecPPOTrainer(N_ENV, T, device=DEV, seed=seed, **CONFIGS[config], **kw)
    if config == "mlp_layered":
        tr.fused_mlp = False
    return tr


@pytest.mark.parametrize("config", ["lstm", "mlp", "lstm_shuffle", "lstm_obs_norm"])
def test_a_pinned_adaptive_rate_is_the_diagnostics_trainer(config):
    """lr_min == lr_max == lr: the rule can never move the rate, so the device-rate Adam path must reproduce the by-value one."""
    a = make(config, diagnostics=True)
    b = make(config, lr_schedule="adaptive", desired_kl=0.01, lr_min=3e-5, lr_max=3e-5)
    assert b.lr_control is not None and a.lr_control is None and b._diag_on
    for _ in range(3):
        a.train_iteration()
        b.train_iteration()
    assert same_optimiser(a, b) and a.opt_step == 3 * 5 * (2 if config == "lstm_shuffle" else 1)
    st = b.lr_control.state.cpu().numpy()
    assert st[0] == 3e-5 and st[2:].sum() == 3.0 and b.learning_rate() == 3e-5
    assert same(b.lr_control.lr_dev, torch.tensor([3e-5], dtype=torch.float32, device=DEV))
    assert same(a._diag_epochs, b._diag_epochs)
    b.losses()


CASES = {"lowered": dict(desired_kl=1e-12, lr_min=1e-5), "raised": dict(desired_kl=1e3, lr_max=1e-4),
         "mid": dict(desired_kl=1e-5, target_kl=1e-7, lr=1e-3)}


def _trajectory(tr, iterations=6):
    """[state after every update()], each checked against adapt_rule on the state before and the row the trainer used."""
    from uavppo.lr_control import adapt_rule
    c, out = tr.lr_control, []
    prev = c.state.cpu().numpy()
    for _ in range(iterations):
        assert tr.learning_rate() == prev[0]
        tr.train_iteration()
        row = tr._diag_epochs[tr._diag_epochs_run - 1].cpu().numpy()
        want = adapt_rule(prev, row, c.desired_kl, c.factor, c.lr_min, c.lr_max)
        prev = c.state.cpu().numpy()
        assert same64(prev, want), (prev, want)
        assert c.lr_dev.cpu().numpy().view(np.uint32)[0] == np.float32(want[0]).view(np.uint32)
        assert row[7] == N_ENV * T and want[1] == row[1] / row[7]
        out.append((prev, tr._diag_epochs_run))
    return out


@pytest.fixture(scope="module")
def constant_after_six():
    """policy.flat of the constant trainer after six iterations, per policy kind (computed once)."""
    out = {}
    for kind in ("lstm", "mlp"):
        tr = make(kind)
        for _ in range(6):
            tr.train_iteration()
        out[kind] = tr.policy.flat.clone()
    return out


@pytest.mark.parametrize("kind", ["lstm", "mlp"])
@pytest.mark.parametrize("case", ["lowered", "raised", "mid"])
def test_the_rate_follows_adapt_rule_through_six_iterations(kind, case, constant_after_six):
    tr = make(kind, lr_schedule="adaptive", **CASES[case])
    assert same64(tr.lr_control.state.cpu().numpy(), [tr.hp["lr"], 0, 0, 0, 0, 0])
    traj = _trajectory(tr)
    last = traj[-1][0]
    if case == "lowered":
        assert last[0] == 1e-5 and last[3] == 6.0 and [s[0] for s, _ in traj[:3]] == [3e-5 / 1.5, 3e-5 / 1.5 / 1.5, 1e-5]
        assert not same(tr.policy.flat, constant_after_six[kind])              # the rate is actually read
    elif case == "raised":
        assert last[0] == 1e-4 and last[2] == 6.0 and [s[0] for s, _ in traj[:3]] == [3e-5 * 1.5, 3e-5 * 1.5 * 1.5, 1e-4]
        assert not same(tr.policy.flat, constant_after_six[kind])
    else:
        assert any(run < 5 for _, run in traj) and tr.diagnostics()["epochs_run"] == traj[-1][1]      # the early stop's row was used
        assert last[2:].sum() == 6.0 and last[5] == 0.0
    assert tr.hp["lr"] == CASES[case].get("lr", 3e-5)                           # the starting value stays
    tr.losses()


LINEAR = dict(lr_schedule="linear", lr_final=1e-6, ent_beta_final=0.0, schedule_iterations=4)


@pytest.mark.parametrize("config", ["lstm", "mlp", "lstm_shuffle", "mlp_rows", "mlp_layered"])
def test_linear_schedules_are_the_constant_trainer_with_the_values_set_by_hand(config):
    from uavppo.lr_control import linear_value
    a, b = make(config, **LINEAR), make(config)
    assert a.lr_control is None and not a._diag_on
    lrs = []
    for k in range(6):
        lr, ent = float(linear_value(3e-5, 1e-6, k, 4)), float(linear_value(0.01, 0.0, k, 4))
        assert a.learning_rate() == lr and a.entropy_beta() == ent
        b.hp["lr"], b.hp["ent_beta"] = lr, ent
        a.train_iteration()
        b.train_iteration()
        assert same(a.loss_sums, b.loss_sums), k
        lrs.append(lr)
    assert same_optimiser(a, b)
    assert lrs[0] == 3e-5 and lrs[4] == lrs[5] and abs(lrs[4] - 1e-6) < 1e-20 and lrs[1] > lrs[2] > lrs[3] > lrs[4]
    assert a.hp["lr"] == 3e-5 and a.hp["ent_beta"] == 0.01                      # the starting values stay
    c = make(config)
    for _ in range(6):
        c.train_iteration()
    assert not same(a.policy.flat, c.policy.flat)                               # the schedule did something


@pytest.mark.parametrize("config", ["lstm", "mlp"])
def test_a_linear_schedule_that_ends_where_it_starts_is_the_untouched_trainer(config):
    a = make(config, lr_schedule="linear", lr_final=3e-5, ent_beta_final=0.01, schedule_iterations=4)
    b = make(config)
    for _ in range(6):
        a.train_iteration()
        b.train_iteration()
    assert same_optimiser(a, b) and same(a.loss_sums, b.loss_sums)


def test_ent_beta_final_works_beside_the_adaptive_rate():
    from uavppo.lr_control import linear_value
    a = make("lstm", lr_schedule="adaptive", desired_kl=0.01, lr_min=3e-5, lr_max=3e-5, ent_beta_final=0.0, schedule_iterations=2)
    b = make("lstm", diagnostics=True)
    for k in range(3):
        b.hp["ent_beta"] = float(linear_value(0.01, 0.0, k, 2))
        assert a.entropy_beta() == b.hp["ent_beta"]
        a.train_iteration()
        b.train_iteration()
    assert same_optimiser(a, b)


_CHILD = """
import json, sys
sys.path[:0] = [%r, %r]
import torch
from uavppo.dist_utils import collectives_on, use_abi_collectives
from uavppo.trainer import VecPPOTrainer
use_abi_collectives(0, 1, "cuda:0")
assert collectives_on()
tr = VecPPOTrainer(64, 16, policy="lstm", hidden=64, device="cuda:0", seed=11, lr_schedule="adaptive", desired_kl=1e-5, target_kl=1e-7, lr=1e-3)
out = []
for _ in range(6):
    tr.train_iteration()
    out.append([tr.lr_control.state.cpu().numpy().view("uint64").tolist(), tr._diag_epochs_run])
tr.losses()
print(json.dumps(out))
"""


def test_the_rate_trajectory_is_the_same_under_forced_one_rank_collectives():
    """The mid case with the diagnostic row's all-reduce issued for real: a one-rank RCCL communicator on the C ABI's carrier with
    UAVPPO_FORCE_COLLECTIVES=1 (process-wide state, hence a child process).  A sum over one rank changes nothing."""
    code = _CHILD % (ROOT, os.path.join(ROOT, "uav-wrf-les-ppo-lstm_amd"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120, env=dict(os.environ, UAVPPO_FORCE_COLLECTIVES="1"))
    assert r.returncode == 0, r.stderr[-2000:]
    forced = json.loads(r.stdout.strip().splitlines()[-1])
    tr = make("lstm", lr_schedule="adaptive", **CASES["mid"])
    plain = []
    for _ in range(6):
        tr.train_iteration()
        plain.append([tr.lr_control.state.cpu().numpy().view(np.uint64).tolist(), tr._diag_epochs_run])
    assert plain == forced


def test_state_dict_round_trip():
    a = make("mlp", lr_schedule="adaptive", desired_kl=1e3, lr_max=1e-4)
    for _ in range(2):
        a.train_iteration()
    sd = a.lr_control.state_dict()
    assert sorted(sd) == ["state"] and sd["state"].dtype == np.float64 and sd["state"].shape == (6,) and sd["state"][2] == 2.0
    b = make("mlp", seed=99, lr_schedule="adaptive", desired_kl=1e3, lr_max=1e-4)
    b.lr_control.load_state_dict(sd)
    assert same(a.lr_control.state, b.lr_control.state) and same(a.lr_control.lr_dev, b.lr_control.lr_dev)
    assert b.learning_rate() == a.learning_rate() == 3e-5 * 1.5 * 1.5
    with pytest.raises(ValueError):
        b.lr_control.load_state_dict({"state": sd["state"][:4]})
    with pytest.raises(ValueError):
        b.lr_control.load_state_dict({"state": np.array([1.0, 0, 0, 0, 0, 0])})        # a rate outside the bounds
    b.reset()
    assert same64(b.lr_control.state.cpu().numpy(), [3e-5, 0, 0, 0, 0, 0])


def test_save_state_writes_lr_state_npz(tmp_path):
    from uavppo.lr_control import STATE_FILE, LrController, save_state
    c = LrController(3e-5, 0.01, device=DEV)
    path = save_state(c, str(tmp_path / "m" / "model.pth"))
    d = np.load(path)
    assert os.path.basename(path) == STATE_FILE == "lr_state.npz" and same64(d["state"], [3e-5, 0, 0, 0, 0, 0])
    assert float(d["desired_kl"]) == 0.01 and float(d["factor"]) == 1.5 and float(d["lr_min"]) == 1e-6 and float(d["lr_max"]) == 1e-2


def _script(name, file, monkeypatch, **cfg):
    """A training script loaded with config names set for the duration of the test (the scripts import them by name)."""
    import importlib.util
    import config
    for k, v in cfg.items():
        assert hasattr(config, k), k
        monkeypatch.setattr(config, k, v)
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "uav-wrf-les-ppo-lstm_amd", file))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_train_script_logs_the_values_each_update_ran_with_and_saves_the_state(tmp_path, monkeypatch):
    """config.LR_SCHEDULE "adaptive" with ENTROPY_BETA_FINAL: update_diagnostics.csv is written without PPO_DIAGNOSTICS, its two
    extra columns hold what each iteration's update ran with, and lr_state.npz lands beside the model."""
    from uavppo.lr_control import linear_value
    cfg = dict(NUM_ENVS=8, HORIZON=16, POLICY="mlp", EPOCHS=3, LR_SCHEDULE="adaptive", DESIRED_KL=1e3, LR_MAX=1e-4,
               ENTROPY_BETA_FINAL=0.0, SCHEDULE_ITERATIONS=2)
    m = _script("train_ppo2_0_lr", "train_ppo2.0.py", monkeypatch, **cfg)
    tr, _ = m.train_ppo_vectorised(iterations=3, csv_path=str(tmp_path / "episodes.csv"), model_path=str(tmp_path / "model.pth"), log_every=0)
    lines = open(tmp_path / "update_diagnostics.csv").read().splitlines()
    assert lines[0].split(",")[-2:] == ["Learning_Rate", "Entropy_Beta"] and len(lines[0].split(",")) == 9 and len(lines) == 4
    got = [[float(v) for v in ln.split(",")[-2:]] for ln in lines[1:]]
    assert got == [[lr, float(linear_value(0.01, 0.0, k, 2))] for k, lr in enumerate((3e-5, 3e-5 * 1.5, 3e-5 * 1.5 * 1.5))]      # raised after every update
    d = np.load(tmp_path / "lr_state.npz")
    assert same64(d["state"], tr.lr_control.state.cpu().numpy()) and d["state"][0] == 1e-4 and d["state"][2] == 3.0
    assert float(d["desired_kl"]) == 1e3 and float(d["lr_max"]) == 1e-4
    # without a schedule the file has the columns it always had
    m = _script("train_ppo2_0_plain", "train_ppo2.0.py", monkeypatch, NUM_ENVS=8, HORIZON=16, POLICY="mlp", EPOCHS=3, PPO_DIAGNOSTICS=True,
                LR_SCHEDULE="constant", DESIRED_KL=None, ENTROPY_BETA_FINAL=None, SCHEDULE_ITERATIONS=None)
    os.makedirs(tmp_path / "b")
    m.train_ppo_vectorised(iterations=1, csv_path=str(tmp_path / "b" / "episodes.csv"), model_path=str(tmp_path / "b" / "model.pth"), log_every=0)
    assert open(tmp_path / "b" / "update_diagnostics.csv").readline().strip().endswith(",Explained_Variance")
    assert not os.path.exists(tmp_path / "b" / "lr_state.npz")


def test_gail_script_passes_the_config_names_through(tmp_path, monkeypatch):
    rng = np.random.RandomState(3)
    np.savez(str(tmp_path / "expert_data.npz"), states=rng.rand(64, 6).astype(np.float32), actions=rng.randint(0, 5, 64).astype(np.int64))
    m = _script("train_ppo_gail_lr", "train_ppo_gail.py", monkeypatch, NUM_ENVS=8, HORIZON=16, EPOCHS=2, PPO_DIAGNOSTICS=True,
                LR_SCHEDULE="linear", LR_FINAL=1e-5, SCHEDULE_ITERATIONS=2)
    tr = m.train_ppo_gail(num_episodes=10 ** 6, num_envs=8, horizon=16, expert_path=str(tmp_path / "expert_data.npz"), policy="mlp",
                          max_iterations=3, model_path=str(tmp_path / "g.pth"), disc_path=str(tmp_path / "d.pth"))
    from uavppo.lr_control import linear_value
    want = [float(linear_value(3e-5, 1e-5, k, 2)) for k in range(4)]
    assert tr.lr_schedule == "linear" and tr.learning_rate() == want[3] == want[2] and tr.lr_control is None
    assert want[0] == 3e-5 and abs(want[1] - 2e-5) < 1e-19 and abs(want[2] - 1e-5) < 1e-19
    lines = open(tmp_path / "update_diagnostics.csv").read().splitlines()
    assert [[float(v) for v in ln.split(",")[-2:]] for ln in lines[1:]] == [[want[k], 0.01] for k in range(3)]
    assert not os.path.exists(tmp_path / "lr_state.npz")


def test_gail_accepts_the_keywords_and_runs():
    from uavppo.gail import GAILTrainer
    rng = np.random.RandomState(31)
    expert = (rng.rand(200, 6).astype(np.float32), rng.randint(0, 5, 200).astype(np.int64))
    tr = GAILTrainer(N_ENV, T, "mlp", device=DEV, seed=5, expert=expert, lr_schedule="adaptive", desired_kl=1e3, lr_max=1e-4,
                     ent_beta_final=0.0, schedule_iterations=2, disc_lr=1e-3)
    for _ in range(2):
        tr.train_iteration()
    tr.losses()
    tr.disc_losses()
    assert tr.learning_rate() == 3e-5 * 1.5 * 1.5 and tr.entropy_beta() == 0.0 and tr.disc_lr == 1e-3 and tr.disc_opt_step == 2
