"""The inline PPO update of PPOV1.1/train_ppo1.0.py on the device: uav_gae mode UAV_GAE_INLINE_V10, uav_adv_normalise_inline,
uav_mlp_ppo_grad_rows, VecPPOTrainer(update_form="inline_v10", minibatch_rows=B), GAILTrainer with the same arguments, and
the package's train_ppo1.0.py -- against the f64 restatement of tests/_inline_update_check.py (which meets the reference's own
recording on the CPU, tests/test_inline_update_host.py), against the contiguous kernels bit for bit, and against the recording
itself.  -m gpu."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import _inline_update_check as iu
from test_gpu_trainer import _redraw_kink_samples

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "uav-wrf-les-ppo-lstm_amd")


@pytest.fixture(scope="module")
def ops():
    from uavppo import ops as o
    return o


def dev(x):
    return torch.as_tensor(np.asarray(x)).to(DEV).contiguous()


def grad_bound(n, scale):
    """tests/test_gpu_trend_mlp.py: f32 sums over n samples on both sides, in different orders."""
    return (2e-5 + 2e-7 * np.sqrt(n)) * scale + 1e-9


# ---------------------------------------------------------------------------------------------- uav_gae mode 2
@pytest.fixture(scope="module")
def gae_cases():
    """Inputs and the f64 restatement's advantages, computed once."""
    out = {}
    for n, T in ((1, 1), (3, 7), (5, 64), (4, 65), (2, 130)):
        rng = np.random.RandomState(n * 1000 + T)
        rew, val = (rng.randn(n, T) * 2).astype(np.float32), rng.randn(n, T).astype(np.float32)
        done = (rng.rand(n, T) < 0.1).astype(np.float32)
        done[:, -1] = np.arange(n) % 2              # done on the very last step for half the rows
        last = rng.randn(n).astype(np.float32)
        f = lambda a: torch.from_numpy(a).double()
        out[(n, T)] = (rew, val, done, last, iu.gae_inline(f(rew), f(val), f(done), f(last)).numpy())
    return out


@pytest.mark.parametrize("n,T", [(1, 1), (3, 7), (5, 64), (4, 65), (2, 130)])
def test_gae_inline_mode_matches_f64_and_leaves_the_other_modes_alone(ops, gae_cases, n, T):
    rew, val, done, last, want = gae_cases[(n, T)]
    r, v, d, lv = dev(rew), dev(val), dev(done), dev(last)
    before = [ops.gae(r, v, d, 0.99, 0.95, "reference_exact"), ops.gae(r, v, d, 0.99, 0.95, "standard", last_val=lv)]
    got = ops.gae(r, v, d, 0.99, 0.95, "inline_v10", last_val=lv).cpu().numpy()
    after = [ops.gae(r, v, d, 0.99, 0.95, "reference_exact"), ops.gae(r, v, d, 0.99, 0.95, "standard", last_val=lv)]
    print("max err", np.abs(got - want).max())
    # f32 tolerance: the wave scan re-associates the recurrence (tests/test_gpu_update_kernels.py)
    assert np.allclose(got, want, rtol=2e-5, atol=2e-5)
    for a, b in zip(before, after):
        assert torch.equal(a, b)
    if T > 1:       # the three modes are three different recurrences on these inputs
        assert not np.array_equal(got, before[0].cpu().numpy()) and not np.array_equal(got, before[1].cpu().numpy())


def test_gae_inline_mode_needs_last_val(ops):
    z = torch.zeros(2, 4, device=DEV)
    with pytest.raises(RuntimeError, match="UAV_GAE_INLINE_V10 needs last_val"):
        ops.gae(z, z, z, 0.99, 0.95, "inline_v10")


# ---------------------------------------------------------------------------------------------- uav_adv_normalise_inline
@pytest.mark.parametrize("n", [2, 257, 70000])
def test_adv_normalise_inline_matches_f64(ops, n):
    rng = np.random.RandomState(n)
    adv, val = (rng.randn(n) * 3 + 1.5).astype(np.float32), rng.randn(n).astype(np.float32)
    a = dev(adv)
    ga, gr = ops.adv_normalise_inline(a, dev(val), ops.adv_stats(a))
    want_a, _ = iu.normalise_inline(torch.from_numpy(adv).double(), torch.from_numpy(val).double())
    assert np.array_equal(gr.cpu().numpy(), adv + val)                   # returns: the f32 sum of the RAW advantage, bit for bit
    # rtol 1e-6 and nothing else: the kernel subtracts the f64 mean, so elements next to the mean meet it too
    err = np.abs(ga.cpu().numpy() - want_a.numpy())
    rel = err / np.abs(want_a.numpy())
    print("max err", err.max(), "max rel err", rel.max(), "smallest |want|", np.abs(want_a.numpy()).min())
    assert (err <= 1e-6 * np.abs(want_a.numpy())).all()


def test_adv_normalise_inline_adds_1e_8_to_the_std(ops):
    """A near-constant buffer, std 2e-6: (std + 1e-8) is 0.5 % above std, uav_adv_normalise's (std + 1e-6) 50 % above it (and
    its guard would divide by 1 below 1e-6), so the constant and the missing guard show at the bound of the test above."""
    rng = np.random.RandomState(3)
    adv, val = (2e-6 * rng.randn(4099)).astype(np.float32), rng.randn(4099).astype(np.float32)
    a = dev(adv)
    stats = ops.adv_stats(a)
    ga, gr = ops.adv_normalise_inline(a, dev(val), stats)
    want_a, _ = iu.normalise_inline(torch.from_numpy(adv).double(), torch.from_numpy(val).double())
    sd = adv.astype(np.float64).std(ddof=1)
    assert 1e-6 < sd < 4e-6
    err = np.abs(ga.cpu().numpy() - want_a.numpy())
    print("std", sd, "max rel err", (err / np.abs(want_a.numpy())).max())
    assert (err <= 1e-6 * np.abs(want_a.numpy())).all() and np.array_equal(gr.cpu().numpy(), adv + val)
    old, _ = ops.adv_normalise(a, dev(val), stats)
    assert not np.allclose(old.cpu().numpy(), want_a.numpy(), rtol=1e-2, atol=0)


def test_adv_normalise_inline_of_one_sample_is_nan(ops):
    a, v = torch.tensor([0.75], device=DEV), torch.tensor([0.5], device=DEV)
    ga, gr = ops.adv_normalise_inline(a, v, ops.adv_stats(a))
    assert torch.isnan(ga).all() and gr.item() == 1.25


# ---------------------------------------------------------------------------------------------- uav_mlp_ppo_grad_rows
def _policy(k, seed):
    from uavppo.policy import MLPActorCritic
    pol = MLPActorCritic(6 + k, 5, device=DEV, seed=seed)
    with torch.no_grad():        # non-trivial LayerNorm parameters and biases (tests/test_gpu_trend_mlp.py)
        g = torch.Generator().manual_seed(1)
        for key in ("feature.0.bias", "feature.1.bias", "feature.3.bias", "feature.4.bias", "head.bias"):
            pol.views[key].copy_(torch.randn(pol.views[key].shape, generator=g) * 0.2)
        for key in ("feature.1.weight", "feature.4.weight"):
            pol.views[key].copy_(1 + 0.3 * torch.randn(pol.views[key].shape, generator=g))
        pol.views["head.weight"].mul_(20.0)
    return pol


def _samples(n, k, seed):
    rng = np.random.RandomState(seed)
    obs = rng.rand(n, 6 + k).astype(np.float32)
    obs[:, 6:] = 0.05 * rng.randn(n, k)
    act = rng.randint(0, 5, n).astype(np.int32)
    adv, ret, vo = (rng.randn(n).astype(np.float32) for _ in range(3))
    lp = (np.log(0.2) + 0.3 * rng.randn(n)).astype(np.float32)
    return obs, act, lp, adv, ret, vo


def _contiguous(ops, pol, k, s, inv_n):
    sums = torch.zeros(4, dtype=torch.float64, device=DEV)
    grad = torch.full_like(pol.flat, float("nan"))
    if k:
        ops.mlp_ppo_grad_trend(pol.flat, *s, inv_n, 0.2, 0.01, sums, grad, k)
    else:
        ops.mlp_ppo_grad(pol.flat, *s, inv_n, 0.2, 0.01, sums, grad)
    return grad, sums


def _by_rows(ops, pol, k, s, rows, inv_n):
    sums = torch.zeros(4, dtype=torch.float64, device=DEV)
    grad = torch.full_like(pol.flat, float("nan"))
    ops.mlp_ppo_grad_rows(pol.flat, *s, rows, inv_n, 0.2, 0.01, sums, grad, k)
    return grad, sums


@pytest.mark.parametrize("mode", ["fp16x3", "f32_mfma"])
@pytest.mark.parametrize("k", [0, 2])
@pytest.mark.parametrize("n", [1, 31, 33, 100, 8300])
def test_grad_rows_with_identity_rows_is_the_contiguous_kernel(ops, n, k, mode):
    """rows = arange(n): gradient and loss sums of uav_mlp_ppo_grad(_trend), bit for bit.  8300 rows are more 32-sample tiles
    than there are CUs: workgroups take a second tile (and prefetch its indices)."""
    pol = _policy(k, 3)
    s = [dev(a) for a in _samples(n, k, n + k)]
    with ops.lstm_arith(mode):
        want = _contiguous(ops, pol, k, s, 1.0 / n)
        got = _by_rows(ops, pol, k, s, torch.arange(n, dtype=torch.int32, device=DEV), 1.0 / n)
    assert torch.isfinite(want[0]).all() and (want[0] != 0).any()
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


@pytest.mark.parametrize("mode", ["fp16x3", "f32_mfma"])
@pytest.mark.parametrize("k", [0, 2])
@pytest.mark.parametrize("n_rows", [7, 33, 8300])
def test_grad_rows_of_a_shuffled_subset_is_the_contiguous_kernel_on_gathered_copies(ops, n_rows, k, mode):
    n_total = 20000
    pol = _policy(k, 4)
    s = [dev(a) for a in _samples(n_total, k, 77 + k)]
    rows = torch.from_numpy(np.random.RandomState(n_rows).permutation(n_total)[:n_rows].astype(np.int32)).to(DEV)
    gathered = [t.index_select(0, rows.long()).contiguous() for t in s]
    with ops.lstm_arith(mode):
        want = _contiguous(ops, pol, k, gathered, 1.0 / n_rows)
        got = _by_rows(ops, pol, k, s, rows, 1.0 / n_rows)
    assert torch.isfinite(want[0]).all() and (want[0] != 0).any()
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    # ... and it is NOT what the first n_rows buffer rows give: the index is read
    with ops.lstm_arith(mode):
        head = _contiguous(ops, pol, k, [t[:n_rows].contiguous() for t in s], 1.0 / n_rows)
    assert not torch.equal(head[0], got[0])


def _named(pol, flat):
    """A flat parameter-layout tensor as the reference's state_dict keys."""
    out, o = {}, 0
    for name, shape in pol.layout:
        cnt = int(np.prod(shape))
        out[name] = flat[o:o + cnt].view(shape)
        o += cnt
    return pol._named(out)


def _check_grad(pol, grad_flat, sums, p64, s64, n):
    want, ls = iu.grad_of(p64, *s64)
    got = {key: v.cpu().double() for key, v in _named(pol, grad_flat).items()}
    got_sums = sums.cpu().numpy()
    print("losses", got_sums[:3] / n, ls[1:])
    assert np.allclose(got_sums[:3] / n, ls[1:], rtol=2e-5, atol=1e-6) and got_sums[3] == 0
    for key in want:
        scale = want[key].abs().max().item() + 1e-12
        err = (got[key] - want[key]).abs().max().item()
        print(key, "err", err, "bound", grad_bound(n, scale))
        assert err <= grad_bound(n, scale), (key, err, scale)


@pytest.mark.parametrize("mode", ["fp16x3", "f32_mfma"])
def test_grad_rows_matches_f64_autograd(ops, mode):
    """100 shuffled rows of a 300-row buffer, trend_k = 2, against autograd in f64 through the restatement: the chain of
    bit-equalities above does not rest on the older kernel alone."""
    n_total, n, k = 300, 100, 2
    pol = _policy(k, 5)
    rng = np.random.RandomState(9)
    obs, act, lp, adv, ret, vo = _samples(n_total, k, 9)
    _redraw_kink_samples(pol, rng, obs, act, lp, vo, ret)
    rows = rng.permutation(n_total)[:n].astype(np.int32)
    with ops.lstm_arith(mode):
        grad, sums = _by_rows(ops, pol, k, [dev(a) for a in (obs, act, lp, adv, ret, vo)], dev(rows), 1.0 / n)
    p64 = {key: v.detach().cpu().double() for key, v in pol.named_views().items()}
    s64 = [torch.from_numpy(a[rows]).double() if a.dtype != np.int32 else torch.from_numpy(a[rows]) for a in (obs, act, lp, adv, ret, vo)]
    _check_grad(pol, grad, sums, p64, s64, n)


def test_grad_rows_refuses_bad_arguments(ops):
    pol = _policy(0, 1)
    s = [dev(a) for a in _samples(10, 0, 1)]
    sums, grad = torch.zeros(4, dtype=torch.float64, device=DEV), torch.zeros_like(pol.flat)
    with pytest.raises(RuntimeError, match="rows"):
        ops.mlp_ppo_grad_rows(pol.flat, *s, torch.arange(4, device=DEV), 0.25, 0.2, 0.01, sums, grad)          # int64 indices
    with pytest.raises(RuntimeError, match="non-empty"):
        ops.mlp_ppo_grad_rows(pol.flat, *s, torch.zeros(0, dtype=torch.int32, device=DEV), 0.25, 0.2, 0.01, sums, grad)
    with pytest.raises(RuntimeError, match="trend_k=3"):
        ops.mlp_ppo_grad_rows(pol.flat, *s, torch.arange(4, dtype=torch.int32, device=DEV), 0.25, 0.2, 0.01, sums, grad, 3)


# ---------------------------------------------------------------------------------------------- trainer
def _trainer(cls=None, **kw):
    from uavppo.trainer import VecPPOTrainer
    tr = (cls or VecPPOTrainer)(8, 32, "mlp", device=DEV, seed=11, use_curriculum=False, epochs=2, **kw)
    tr.radius = 150.0            # episodes end inside the 32 steps
    tr.reset()
    return tr


def _state(tr):
    return [tr.policy.flat, tr.exp_avg, tr.exp_avg_sq, tr.adv_n, tr.ret, tr.loss_sums] + [tr.buf[k] for k in sorted(tr.buf)]


def test_trainer_inline_update_in_row_minibatches(ops):
    """N = 8, T = 32, minibatch_rows = 100: 3 chunks per epoch, the last of 56 rows.  Advantages / returns and the gradient of
    every optimiser step (at the parameters logged with it) against the f64 restatement; and trainers built with the defaults
    before and after are bit-identical: nothing leaked into the default path."""
    N, T, B = 8, 32, 100
    d0 = _trainer()
    for _ in range(2):
        d0.train_iteration()
    tr = _trainer(update_form="inline_v10", minibatch_rows=B)
    assert tr.last_val is not None and tr.gae_mode == "inline_v10"
    g = torch.Generator().manual_seed(5)
    perms = [torch.randperm(N * T, generator=g) for _ in range(2)]
    tr.forced_perms = [p.clone() for p in perms]
    tr.record = tr.record_grads = True
    tr.collect()
    tr.update()
    assert tr.forced_perms == [] and len(tr.grad_log) == 6 and tr.opt_step == 6
    b = {k: v.cpu() for k, v in tr.buf.items()}
    assert b["done"].sum() >= 2
    f = lambda t: t.double()
    adv = iu.gae_inline(f(b["rew"]), f(b["val"]), f(b["done"]), f(tr.last_val.cpu()))
    adv_n, ret = iu.normalise_inline(adv, f(b["val"]))
    # the GAE's tolerance (tests/test_gpu_update_kernels.py) on the raw advantage, carried through (A - mean) / std: the mean
    # and the std each move by at most that much
    delta = 2e-5 * (1 + adv.abs().max().item())
    assert np.allclose(tr.adv.cpu().numpy(), adv.numpy(), rtol=2e-5, atol=2e-5)
    assert (tr.ret.cpu().double() - ret).abs().max().item() <= delta
    sd = adv.std().item()
    err = (tr.adv_n.cpu().double() - adv_n).abs()
    print("adv_n max err", err.max().item(), "bound", 2 * delta / sd)
    assert (err <= 2 * delta / sd + (delta / sd) * adv_n.abs()).all()
    # every optimiser step: the chunk, its gradient, its loss sums
    flat = [b["obs"].reshape(-1, 6), b["act"].reshape(-1), b["logp"].reshape(-1), tr.adv_n.cpu().reshape(-1), tr.ret.cpu().reshape(-1),
            b["val"].reshape(-1)]
    sizes = []
    for i, (grad, params) in enumerate(tr.grad_log):
        idx = perms[i // 3].split(B)[i % 3]
        sizes.append(len(idx))
        p64 = {key: v.cpu().double() for key, v in _named(tr.policy, params).items()}
        s64 = [t[idx].double() if t.dtype != torch.int32 else t[idx] for t in flat]
        _check_grad(tr.policy, grad, tr.log[i][0], p64, s64, len(idx))
    assert sizes == [100, 100, 56] * 2
    # losses() divides by the last chunk's size
    want = tr.log[-1][0].cpu().numpy()[:3] / 56
    assert np.allclose(tr.losses(), want, rtol=1e-12)
    # a drawn permutation: device generator seeded by (seed, rank); two trainers agree, and every row is visited once
    a, c = _trainer(update_form="inline_v10", minibatch_rows=B), _trainer(update_form="inline_v10", minibatch_rows=B)
    pa = a._next_perm()
    assert pa.dtype == torch.int32 and torch.equal(pa, c._next_perm()) and torch.equal(pa.sort().values.cpu(), torch.arange(N * T, dtype=torch.int32))
    pb = a._next_perm()
    assert not torch.equal(pa, pb) and torch.equal(pb, c._next_perm())           # the generator moves on, alike in both
    for t_ in (a, c):
        t_.train_iteration()
    assert all(torch.equal(x, y) for x, y in zip(_state(a), _state(c))) and a.opt_step == 6
    # the default path, after all that
    d1 = _trainer(update_form="update_model", minibatch_rows=None)
    for _ in range(2):
        d1.train_iteration()
    assert all(torch.equal(x, y) for x, y in zip(_state(d0), _state(d1)))
    assert d0.losses() == d1.losses() and d0.last_val is None


def test_trainer_refuses_row_minibatches_where_they_do_not_exist():
    from uavppo.trainer import VecPPOTrainer
    with pytest.raises(ValueError, match="MLP policy on the fused path"):
        VecPPOTrainer(8, 32, "lstm", hidden=64, device=DEV, minibatch_rows=100)
    with pytest.raises(ValueError, match="give one of them"):
        VecPPOTrainer(8, 32, "mlp", device=DEV, minibatch_rows=100, num_minibatches=2)
    with pytest.raises(ValueError, match="update_form"):
        VecPPOTrainer(8, 32, "mlp", device=DEV, update_form="inline")
    with pytest.raises(ValueError, match="gae_mode='standard' would be ignored"):
        VecPPOTrainer(8, 32, "mlp", device=DEV, update_form="inline_v10", gae_mode="standard")


def test_gail_trainer_inherits_the_inline_update():
    """gail_coef = 0, env_coef = 1: GAILTrainer(update_form="inline_v10", minibatch_rows=...) is VecPPOTrainer with the same
    arguments, bit for bit."""
    from uavppo.gail import GAILTrainer
    rng = np.random.RandomState(61)
    expert = (rng.rand(300, 6).astype(np.float32), rng.randint(0, 5, 300).astype(np.int64))
    kw = dict(update_form="inline_v10", minibatch_rows=100)
    a = _trainer(**kw)
    b = _trainer(GAILTrainer, expert=expert, env_coef=1.0, gail_coef=0.0, **kw)
    for _ in range(2):
        a.train_iteration()
        b.train_iteration()
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(_state(a), _state(b)))
    assert a.losses() == b.losses() and a.opt_step == b.opt_step == 12 and b.disc_opt_step == 2


def test_train_ppo_gail_entry_passes_the_two_arguments_on(tmp_path):
    import sys
    if PKG not in sys.path:
        sys.path.insert(0, PKG)
    import train_ppo_gail as tg
    rng = np.random.RandomState(5)
    np.savez(str(tmp_path / "expert_data.npz"), states=rng.rand(200, 6).astype(np.float32), actions=rng.randint(0, 5, 200))
    tr = tg.train_ppo_gail(10 ** 6, 8, 32, str(tmp_path / "expert_data.npz"), "mlp", max_iterations=2, model_path=None, disc_path=None,
                           update_form="inline_v10", minibatch_rows=100)
    assert tr.update_form == "inline_v10" and tr.minibatch_rows == 100 and tr.opt_step == 2 * tr.hp["epochs"] * 3
    assert torch.isfinite(tr.policy.flat).all() and np.isfinite(tr.losses()).all()


# ---------------------------------------------------------------------------------------------- the script
def _script():
    spec = importlib.util.spec_from_file_location("train_ppo1_0", os.path.join(PKG, "train_ppo1.0.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.mark.parametrize("opt_kind", ["clip_adam", "torch_adam"])
def test_update_inline_replays_the_reference_recording(golden, opt_kind):
    """The three recorded buffers, V(next_state)s and permutations of the reference's own train_ppo1.0.py run through
    _update_inline(buffer, next_value, model, optimizer, perms): every post-update state_dict to atol 4e-7."""
    from model import PPOActorCritic, PPOBuffer
    tr = _script()
    g = golden("update_v10.npz")
    E = int(g["epochs"])
    m = PPOActorCritic(6, 5)
    m.load_state_dict({k: torch.from_numpy(g["sd." + k][0]) for k in iu.KEYS})
    opt = tr.ClipAdam(m.parameters(), lr=float(g["lr"])) if opt_kind == "clip_adam" else torch.optim.Adam(m.parameters(), lr=float(g["lr"]))
    for u in range(3):
        buf = PPOBuffer()
        for i in range(g["states"].shape[1]):
            buf.store(g["states"][u, i], g["actions"][u, i], g["rewards"][u, i], g["values"][u, i], g["log_probs"][u, i], g["dones"][u, i])
        perms = [torch.from_numpy(g["perms"][u * E + e]) for e in range(E)]
        steps = tr._update_inline(buf, torch.tensor(g["next_value"][u]), m, opt, perms)
        assert perms == [] and [n for _, n in steps] == [256] * E
        for e, (sums, n) in enumerate(steps):
            s = sums.cpu().numpy() / n
            total = s[0] + s[1] - 0.01 * s[2]
            print("update", u, "epoch", e, "loss", total, "want", g["loss"][u * E + e])
            assert abs(total - g["loss"][u * E + e]) <= 2e-5 * max(1.0, abs(g["loss"][u * E + e]))      # the loss sums' rtol above
        sd = m.state_dict()
        for k in iu.KEYS:
            err = np.abs(sd[k].cpu().numpy() - g["sd." + k][u + 1]).max()
            print("update", u, k, "err", err)
            assert err <= 4e-7, (u, k, err)


def test_train_ppo_v10_script_runs_300_steps():
    tr = _script()
    model, saved, trainer = tr.train_ppo(episodes=50, max_steps_total=300)
    sd = model.state_dict()
    assert all(torch.isfinite(v).all() for v in sd.values()) and isinstance(saved, list)
    from model import PPOActorCritic
    fresh = PPOActorCritic(6, 5).state_dict()
    assert list(sd) == list(fresh)
    n = trainer.optimizer.step_count                 # an update per BATCH_SIZE = 256 rows: EPOCHS one-chunk epochs each
    assert n >= 5 and n % 5 == 0
