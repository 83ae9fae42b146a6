"""Update diagnostics (uav_set_ppo_diag) and the KL-target early stop on the device: the five loss-bearing entry points with a
buffer attached against detached (every other output bit for bit, the eight sums against the f64 restatement of
tests/_ppo_diag_check.py), detaching, the trainer with diagnostics on against off, the early stop against a run of fewer
epochs, and two ranks over gloo.  -m gpu."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _ppo_diag_check as dc
from conftest import PKG, ROOT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")


@pytest.fixture(scope="module")
def ops():
    from uavppo import ops as o
    return o


@pytest.fixture(scope="module")
def cases():
    """Inputs and the restatement's sums, computed once and left unchanged."""
    return {k: f() for k, f in dc.CASES.items()}


def dev(x):
    return torch.as_tensor(np.asarray(x)).to(DEV).contiguous()


def _nan(*shape, dtype=torch.float32):
    return torch.full(shape, NAN, dtype=dtype, device=DEV)


# ---------------------------------------------------------------------------------------------- 1: the five routes
def _run_route(ops, c, layout):
    """One call of the case's entry point into fresh NaN-filled outputs; returns them (loss sums first)."""
    sums = _nan(4, dtype=torch.float64)
    s = [dev(c[k]) for k in ("act", "logp_old", "adv", "ret", "val_old")]
    n = len(c["act"])
    if layout == "split":
        dz, dv, db = _nan(n, 5), _nan(n), _nan(6)
        ops.ppo_loss(dev(c["logits"]), dev(c["value"]), *s, 1.0 / n, dc.CLIP, 0.01, sums, dz, dv, db)
        return [sums, dz, dv, db]
    if layout == "packed":
        heads = dev(np.concatenate([c["logits"], c["value"][:, None]], 1))
        dh, db = _nan(n, 6), _nan(6)
        ops.ppo_loss_heads(heads, *s, 1.0 / n, dc.CLIP, 0.01, sums, dh, db)
        return [sums, dh, db]
    if layout == "from_y":
        dh, db = _nan(n, 6), _nan(6)
        ops.ppo_loss_from_y(dev(c["y"]), dev(c["w_head"]), dev(c["b_head"]), *s, 1.0 / n, dc.CLIP, 0.01, sums, dh, db)
        return [sums, dh, db]
    params, obs = dev(c["params"]), dev(c["obs"])
    grad = torch.full_like(params, NAN)
    k = obs.shape[1] - 6
    if layout == "mlp_rows":
        rows = dev(c["rows"])
        ops.mlp_ppo_grad_rows(params, obs, *s, rows, 1.0 / rows.numel(), dc.CLIP, 0.01, sums, grad, k)
    elif k:
        ops.mlp_ppo_grad_trend(params, obs, *s, 1.0 / n, dc.CLIP, 0.01, sums, grad, k)
    else:
        ops.mlp_ppo_grad(params, obs, *s, 1.0 / n, dc.CLIP, 0.01, sums, grad)
    return [sums, grad]


ROUTES = [("heads_n1", "split"), ("heads_n1", "packed"), ("heads_n1000", "split"), ("heads_n1000", "packed"),
          ("from_y_h64", "from_y"), ("from_y_h128", "from_y"), ("mlp_k0_n1", "mlp"), ("mlp_k0_n33", "mlp"),
          ("mlp_k2_n1", "mlp"), ("mlp_k2_n33", "mlp"), ("mlp_rows", "mlp_rows")]


@pytest.mark.parametrize("name,layout", ROUTES)
def test_route_attached_against_detached(ops, cases, name, layout):
    """Attached: loss sums, dlogits / dheads, dhead_bias and the flat gradient are the detached call's bit for bit, the eight
    sums meet the f64 restatement (counts exactly -- no sample of these inputs lies within 1e-5 of a clip boundary,
    tests/test_ppo_diag_host.py -- the rest to the loss sums' tolerance of test_ppo_loss_fwd_bwd) and repeat bit for bit."""
    c = cases[name]
    assert c["margin"] > dc.MARGIN
    want = _run_route(ops, c, layout)
    diag = _nan(8, dtype=torch.float64)
    ops.set_ppo_diag(diag)
    try:
        got = _run_route(ops, c, layout)
        d1 = diag.clone()
        diag.fill_(NAN)
        again = _run_route(ops, c, layout)
        d2 = diag.clone()
    finally:
        ops.set_ppo_diag(None)
    for w, g, a in zip(want, got, again):
        assert torch.isfinite(w).all()
        assert torch.equal(w, g) and torch.equal(w, a)
    assert want[0][3].item() == 0
    assert torch.equal(d1, d2), (d1, d2)                      # fixed-order reduction: run to run, bit for bit
    n = int(c["ref"][7])
    print(name, layout, "n", n)
    bad = dc.compare(d1.cpu().numpy(), c["ref"], n)
    assert not bad, bad
    assert d1[1].item() >= 0.0                                # k3: every term is non-negative


# ---------------------------------------------------------------------------------------------- 3: detaching
def test_detaching_restores_the_calls_without_diagnostics(ops, cases):
    """After set_ppo_diag(None) a call of each kind leaves the (poisoned) former buffer untouched; a new handle has nothing
    attached, so the calls before any attach never wrote one either."""
    diag = _nan(8, dtype=torch.float64)
    ops.set_ppo_diag(diag)
    try:
        _run_route(ops, cases["heads_n1"], "split")
        assert torch.isfinite(diag).all() and diag[7].item() == 1.0
    finally:
        ops.set_ppo_diag(None)
    diag.fill_(-777.0)
    for name, layout in (("heads_n1000", "packed"), ("from_y_h64", "from_y"), ("mlp_k0_n33", "mlp"), ("mlp_rows", "mlp_rows")):
        _run_route(ops, cases[name], layout)
    torch.cuda.synchronize()
    assert (diag == -777.0).all()


def test_set_ppo_diag_checks_its_buffer(ops):
    with pytest.raises(RuntimeError, match="diag"):
        ops.set_ppo_diag(torch.zeros(8, dtype=torch.float32, device=DEV))
    with pytest.raises(RuntimeError, match="diag"):
        ops.set_ppo_diag(torch.zeros(7, dtype=torch.float64, device=DEV))
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ops.set_ppo_diag(torch.zeros(8, dtype=torch.float64))
    ops.set_ppo_diag(None)


# ---------------------------------------------------------------------------------------------- 4: the trainer, on against off
def _trainer(kind, **kw):
    from uavppo.trainer import VecPPOTrainer
    tr = VecPPOTrainer(8, 16, kind, hidden=64, device=DEV, seed=11, use_curriculum=False, **kw)
    tr.radius = 150.0
    tr.reset()
    return tr


def _state(tr):
    return [tr.policy.flat, tr.exp_avg, tr.exp_avg_sq]


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(_state(a), _state(b))) and a.opt_step == b.opt_step


# |lr| of epoch 0, where the update's parameters ARE the rollout's and only the two flavours of the log-probability differ
# (csrc/loss_core.h: the fused rollouts draw with the hardware __expf / __logf, the loss recomputes with libm's expf / logf):
#   q_a = p_a / sum p, p_k = exp(x_k), x_k = z_k - max z <= 0.  libm expf: 1 ulp = 2^-23 relative.  __expf(x) = v_exp_f32(x log2 e):
#   1 ulp of the instruction + the rounding of its argument, |x| log2(e) 2^-24 relative: <= 2^-23 (1 + 1.443 |x|).  In the sum
#   p_k weighs term k and |x| e^x <= 1 / e, so sum p carries <= 2^-23 (1 + 1.443 * 5 / e) = 3.7 * 2^-23; the taken action's own
#   term, with |x_a| <= |log q_a| < 4 (asserted below), <= 6.8 * 2^-23; the two divisions 2^-23 more: log q_a moves by
#   <= 11.5 * 2^-23 = 1.4e-6 between the flavours.  The logarithm: logf 1 ulp of a value below 4 = 2.4e-7; __logf = v_log_f32
#   (1 ulp of |log2 q| < 6: 4.8e-7) * ln 2, rounded: <= 5.8e-7.  The loss's f32 subtraction logp - logp_old: 2.4e-7.
#   Together |lr| <= 2.5e-6; LR0_MAX allows 4e-6.  k3 = expm1(lr) - lr <= lr^2 / 2 * (1 + |lr|) < 8.1e-12.
LR0_MAX = 4e-6
K3_EPOCH0_MAX = 0.5 * LR0_MAX ** 2 * (1 + LR0_MAX)


@pytest.mark.parametrize("kind", ["lstm", "mlp"])
def test_trainer_with_diagnostics_is_the_trainer_without(ops, kind):
    """8 envs x 16 steps, LSTM h = 64 / the fused MLP, two iterations: parameters and both Adam moments bit for bit.  Epoch 0
    of an update runs on the rollout's own parameters: no ratio and no value has left its clip range (both fractions exactly 0)
    and the approximate KL is bounded by the last-bits difference of the two log-probability flavours (above)."""
    off, on = _trainer(kind), _trainer(kind, diagnostics=True)
    for tr in (off, on):
        for _ in range(2):
            tr.train_iteration()
    assert _same(off, on) and torch.equal(off.loss_sums, on.loss_sums)
    assert on.opt_step == 10
    with pytest.raises(RuntimeError, match="diagnostics=True"):
        off.diagnostics()
    d = on.diagnostics()
    print(kind, d)
    assert d["epochs_run"] == 5 and d["stopped_early"] is False
    assert all(len(d[k]) == 5 and np.isfinite(d[k]).all() for k in ("approx_kl", "approx_kl_k1", "clip_fraction",
                                                                    "value_clip_fraction", "explained_variance"))
    assert on.buf["logp"].abs().max().item() < 4.0                       # the premise of LR0_MAX
    assert d["clip_fraction"][0] == 0.0 and d["value_clip_fraction"][0] == 0.0
    assert 0.0 <= d["approx_kl"][0] <= K3_EPOCH0_MAX and abs(d["approx_kl_k1"][0]) <= LR0_MAX
    assert all(v >= 0.0 for v in d["approx_kl"]) and all(v <= 1.0 for v in d["explained_variance"])
    # the handle is left detached: a loss call of the caller's own writes no buffer of the trainer's
    before = on._diag_sums.clone()
    _run_route(ops, dc.heads_case(8, 1), "split")
    assert torch.equal(before, on._diag_sums)


# ---------------------------------------------------------------------------------------------- 5: the early stop
CUTS = {"envs": ("lstm", dict(num_minibatches=2, shuffle_envs=True), 2),
        "rows": ("mlp", dict(minibatch_rows=50), 3)}          # 128 rows in chunks of 50: 3 optimiser steps per epoch


def _one_update(kind, **kw):
    tr = _trainer(kind, lr=1e-2, **kw)
    tr.collect()
    tr.update()
    return tr


def _pick_target(kl):
    """(e, target): the first epoch e >= 1 whose KL exceeds all earlier ones, and a target halfway between that KL and the
    largest earlier one -- epochs 0 .. e - 1 stay below it, epoch e is over it, whatever the numbers are."""
    for e in range(1, len(kl)):
        if kl[e] > max(kl[:e]):
            return e, 0.5 * (kl[e] + max(kl[:e]))
    raise AssertionError(f"the KL never grew: {kl}")


@pytest.mark.parametrize("cut", sorted(CUTS))
def test_early_stop_is_the_update_of_fewer_epochs(cut):
    kind, kw, steps = CUTS[cut]
    a = _one_update(kind, diagnostics=True, epochs=5, **kw)
    kl = a.diagnostics()["approx_kl"]
    e, target = _pick_target(kl)
    print(cut, "kl", kl, "e", e, "target", target)
    assert e + 1 < 5, "the stop must leave epochs undone"
    b = _one_update(kind, target_kl=target, epochs=5, **kw)
    d = b.diagnostics()
    assert d["epochs_run"] == e + 1 and d["stopped_early"] is True and b.opt_step == (e + 1) * steps
    assert d["approx_kl"] == kl[:e + 1]                                  # the same update up to the stop, bit for bit
    c = _one_update(kind, epochs=e + 1, **kw)
    assert _same(b, c)
    never, plain = _one_update(kind, target_kl=1e30, epochs=5, **kw), _one_update(kind, epochs=5, **kw)
    assert _same(never, plain) and _same(a, plain) and plain.opt_step == 5 * steps
    dn = never.diagnostics()
    assert dn["epochs_run"] == 5 and dn["stopped_early"] is False and dn["approx_kl"] == kl
    # the parameter-range push at the end of update() happened in the stopped run too
    assert len(b.guard.ring) == len(plain.guard.ring) == 1


# ---------------------------------------------------------------------------------------------- 6: two ranks
WORKER = r'''
import os, sys, torch
import torch.distributed as dist
sys.path[:0] = [ROOT, PKG]
from uavppo.trainer import VecPPOTrainer
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
torch.cuda.set_device(0)
if world > 1:
    dist.init_process_group("gloo", rank=rank, world_size=world)

def run(**kw):
    tr = VecPPOTrainer(8 // world, 16, "lstm", hidden=64, device="cuda:0", seed=11, rank=rank, world_size=world, use_curriculum=False,
                       lr=1e-2, epochs=5, **kw)
    tr.radius = 150.0
    tr.reset()
    tr.collect()
    tr.update()
    return tr

target = os.environ.get("TARGET_KL")
if target is None:                 # one rank: the per-epoch KL first, then the target the stop is tested with
    kl = run(diagnostics=True).diagnostics()["approx_kl"]
    e = next(e for e in range(1, 5) if kl[e] > max(kl[:e]))
    target = 0.5 * (kl[e] + max(kl[:e]))
tr = run(target_kl=float(target))
torch.save({"target": float(target), "diag": tr.diagnostics(), "opt_step": tr.opt_step, "flat": tr.policy.flat.cpu()},
           os.environ["OUT"] + f".{rank}")
if dist.is_initialized():
    dist.barrier(); dist.destroy_process_group()
'''


def _run(world, out, port, **extra):
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), OUT=out, **extra)
        procs.append(subprocess.Popen([sys.executable, "-c", f"ROOT={ROOT!r}; PKG={PKG!r}\n" + WORKER], env=env))
    for p in procs:
        assert p.wait(timeout=300) == 0


def test_two_ranks_stop_together(tmp_path):
    """Two ranks share the GPU over gloo, 4 envs each, against one rank with all 8 (tests/test_gpu_multirank.py's pattern): the
    stop is decided from the all-reduced sums, so both ranks report the same epochs_run and the same diagnostics, bit for bit,
    and leave update() together (their processes end, inside the limit); and they are the one-rank run's to the tolerance of
    the existing two-rank tests (rtol 1e-3 on derived scalars, 1e-5 absolute).  The explained variance is compared as the
    ratio it is made of, 1 - EV = sum (R - V)^2 / sum (R - mean R)^2: right after a rollout the critic explains almost nothing
    and EV is the difference of two numbers near 1 (measured: -0.005942 on one rank, -0.005913 on two -- 2.9e-5 apart, 2.9e-5
    relative on the ratio).  rtol 1e-3 of EV itself would be 6e-6, i.e. 6e-6 relative on the sums, from parameters that
    tests/test_gpu_multirank.py allows to differ by a tenth of an Adam step between the two shardings."""
    port = 29900 + os.getpid() % 1000
    _run(1, str(tmp_path / "w1"), port)
    one = torch.load(tmp_path / "w1.0")
    _run(2, str(tmp_path / "w2"), port + 1, TARGET_KL=repr(one["target"]))
    a, b = torch.load(tmp_path / "w2.0"), torch.load(tmp_path / "w2.1")
    print("one", one["diag"], "\ntwo", a["diag"])
    assert a["diag"] == b["diag"] and a["opt_step"] == b["opt_step"] and torch.equal(a["flat"], b["flat"])
    assert one["diag"]["stopped_early"] and 1 < one["diag"]["epochs_run"] < 5
    assert a["diag"]["epochs_run"] == one["diag"]["epochs_run"] and a["diag"]["stopped_early"] and a["opt_step"] == one["opt_step"]
    for k in ("approx_kl", "approx_kl_k1", "clip_fraction", "value_clip_fraction"):
        assert np.allclose(a["diag"][k], one["diag"][k], rtol=1e-3, atol=1e-5), (k, a["diag"][k], one["diag"][k])
    unexplained = [1.0 - np.asarray(d["diag"]["explained_variance"]) for d in (a, one)]
    assert np.allclose(unexplained[0], unexplained[1], rtol=1e-3, atol=1e-5), unexplained


# ---------------------------------------------------------------------------------------------- the scripts
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


def test_train_script_writes_update_diagnostics_csv(tmp_path, monkeypatch, capsys):
    """config.PPO_DIAGNOSTICS: train_ppo_vectorised writes update_diagnostics.csv beside the episode CSV -- one row per
    iteration: the iteration, epochs_run and the last run epoch's five values -- and prints them on its progress line; the
    episode CSV keeps its columns.  With TARGET_KL below any positive KL every update stops early (after the first epoch whose
    KL is not exactly zero: epoch 0 of the fused MLP recomputes the rollout's own log-probabilities)."""
    os.makedirs(tmp_path / "a")
    os.makedirs(tmp_path / "b")
    cfg = dict(NUM_ENVS=8, HORIZON=16, POLICY="mlp", EPOCHS=3, LEARNING_RATE=1e-2)
    m = _script("train_ppo2_0_diag", "train_ppo2.0.py", monkeypatch, PPO_DIAGNOSTICS=True, **cfg)
    tr, _ = m.train_ppo_vectorised(iterations=2, csv_path=str(tmp_path / "a" / "episodes.csv"), model_path=None, log_every=1)
    lines = open(tmp_path / "a" / "update_diagnostics.csv").read().splitlines()
    assert lines[0] == "Iteration,Epochs_Run,Approx_Kl,Approx_Kl_K1,Clip_Fraction,Value_Clip_Fraction,Explained_Variance"
    assert len(lines) == 3 and [ln.split(",")[:2] for ln in lines[1:]] == [["1", "3"], ["2", "3"]]
    last = tr.diagnostics()
    assert [float(v) for v in lines[2].split(",")[2:]] == [last[k][-1] for k in ("approx_kl", "approx_kl_k1", "clip_fraction",
                                                                                "value_clip_fraction", "explained_variance")]
    assert open(tmp_path / "a" / "episodes.csv").readline().strip() == ",".join(m.COLUMNS)
    out = capsys.readouterr().out
    assert out.count("| kl ") == 2 and "epochs 3" in out
    m = _script("train_ppo2_0_kl", "train_ppo2.0.py", monkeypatch, TARGET_KL=1e-30, **cfg)
    tr, _ = m.train_ppo_vectorised(iterations=2, csv_path=str(tmp_path / "b" / "episodes.csv"), model_path=None, log_every=0)
    lines = open(tmp_path / "b" / "update_diagnostics.csv").read().splitlines()
    assert len(lines) == 3 and all(int(ln.split(",")[1]) < 3 for ln in lines[1:])
    assert tr.diagnostics()["stopped_early"]


def test_inline_update_script_collects_diagnostics(monkeypatch):
    """train_ppo1.0.py's _update_inline with a diag_out list: the update's steps and parameters are those without it, the dict
    has one entry per epoch, and config.TARGET_KL stops it."""
    from model import PPOActorCritic, PPOBuffer
    sd0 = {k: v.clone() for k, v in PPOActorCritic(6, 5).state_dict().items()}

    def run(diag, **cfg):
        m = _script("train_ppo1_0_diag", "train_ppo1.0.py", monkeypatch, EPOCHS=3, BATCH_SIZE=64, LEARNING_RATE=1e-2, **cfg)
        model = PPOActorCritic(6, 5)
        model.load_state_dict(sd0)
        opt = m.ClipAdam(model.parameters(), lr=1e-2)
        buf = PPOBuffer()
        r = np.random.RandomState(7)
        for i in range(150):
            buf.store(r.rand(6).astype(np.float32), int(r.randint(5)), float(r.randn()), float(r.randn()), float(np.log(0.2) + 0.05 * r.randn()),
                      bool(i % 50 == 49))
        out = [] if diag else None
        perms = [torch.from_numpy(np.random.RandomState(e).permutation(150)) for e in range(3)]
        steps = m._update_inline(buf, torch.tensor([0.1]), model, opt, perms, diag_out=out)
        return steps, model.core.flat.clone(), out

    s0, p0, _ = run(False)
    s1, p1, out = run(True, PPO_DIAGNOSTICS=True)
    assert torch.equal(p0, p1) and len(s0) == len(s1) == 9 and all(torch.equal(a[0], b[0]) for a, b in zip(s0, s1))
    d = out[0]
    assert d["epochs_run"] == 3 and not d["stopped_early"] and len(d["approx_kl"]) == 3 and all(v > 0 for v in d["approx_kl"])
    s2, _, out = run(True, TARGET_KL=1e-30)
    assert len(s2) == 3 and out[0]["epochs_run"] == 1 and out[0]["stopped_early"]
