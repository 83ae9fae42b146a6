"""Running observation normalisation folded into the first layer, on the GPU: the five kernels of csrc/obs_norm.hip through
uavppo.ops against the numpy statements of uavppo/obs_norm.py (batch_stats, merge_running, fold, unfold_grad, unfold), and
ObsNormaliser inside VecPPOTrainer and GAILTrainer.  -m gpu.

Bars.  Statistics: bit-equal to batch_stats, which sums in the kernel's own order (the file is compiled without FMA contraction and
every product of two f32 values is exact in f64).  Merge: 4 ulp of f64 on the state (the same f64 operations in the same order;
sqrt and the division may differ in the last place), 1 ulp of f32 on mu and inv_sigma.  Fold / unfold_grad / unfold: 1 ulp of f32.
Trainer gradient: see test_the_gradient_is_the_gradient_of_the_normalised_policy."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ops():
    from uavppo import ops as o
    return o


def dev(x, dtype=None):
    t = torch.as_tensor(x)
    return (t if dtype is None else t.to(dtype)).to(DEV).contiguous()


def _obs(rng, rows, D):
    """Observations as the environment scales them: O(1) channels, o[2] in [0, 100] with both ends present."""
    x = rng.standard_normal((rows, D)).astype(np.float32)
    x[:, 2] = (rng.random(rows) * 100.0).astype(np.float32)
    x[0, 2] = 0.0
    x[-1, 2] = 100.0
    return x


def _ulps(a, b):
    """Largest distance of two f32 arrays in units in the last place (values of one sign, or both tiny)."""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    assert a.shape == b.shape
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia, ib = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia), np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)      # sign-magnitude -> a line
    return int(np.abs(ia - ib).max())


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32 if t.dtype == torch.float32 else np.uint64)


# ------------------------------------------------------------------------------------------------ 1: statistics
@pytest.mark.parametrize("rows,D", [(1, 6), (15, 7), (257, 8), (4097, 6), (70001, 7)])       # one row; odd; more than one block;
def test_stats_are_batch_stats_bit_for_bit(ops, rows, D):                                   # every block; more than one row per slot
    from uavppo.obs_norm import batch_stats
    x = _obs(np.random.default_rng(rows), rows, D)
    t = dev(x)
    st = ops.obs_stats(t)
    again = ops.obs_stats(t, torch.full((1 + 2 * D,), float("nan"), dtype=torch.float64, device=DEV))
    got, want = st.cpu().numpy(), batch_stats(x)
    print(f"rows={rows} D={D}: max |got - want| = {np.abs(got - want).max():.3g}")
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    assert np.array_equal(_bits(again), _bits(st))                          # two calls: the same bits
    assert np.array_equal(t.cpu().numpy().view(np.uint32), x.view(np.uint32))            # the input stays
    assert x[:, 2].max() == 100.0 and (rows == 1 or x[:, 2].min() == 0.0)


def test_stats_of_a_strided_view_and_of_a_rollout_buffer(ops):
    from uavppo.obs_norm import batch_stats
    rng = np.random.default_rng(3)
    base = rng.standard_normal((300, 10)).astype(np.float32)
    base[:, 2] = rng.random(300).astype(np.float32) * 100.0
    t = dev(base)
    view = t[:, :7]
    assert not view.is_contiguous()
    got = ops.obs_stats(view).cpu().numpy()
    assert np.array_equal(got.view(np.uint64), batch_stats(base[:, :7]).view(np.uint64))
    buf = _obs(rng, 8 * 16, 6).reshape(8, 16, 6)                            # [N][T][D] is its N T rows
    assert np.array_equal(ops.obs_stats(dev(buf)).cpu().numpy().view(np.uint64), batch_stats(buf.reshape(-1, 6)).view(np.uint64))
    with pytest.raises(RuntimeError):
        ops.obs_stats(t.t()[:7].t()[:, ::2])                                # channels not adjacent


# ------------------------------------------------------------------------------------------------ 2: merge
def _merge_close(got_state, got_mu, got_inv, ref_state, ref_mu, ref_inv):
    for g, r in zip(got_state, ref_state):                 # 4 ulp of f64: the division may differ in the last place, nothing is reordered
        assert abs(g - r) <= 4 * 2.0 ** -52 * abs(r), (got_state, ref_state)
    assert _ulps(got_mu, ref_mu) <= 1 and _ulps(got_inv, ref_inv) <= 1, (got_mu, ref_mu, got_inv, ref_inv)


def _merge(ops, state, stats, D, mask=None, eps=1e-4):
    mu, inv = torch.full((D,), 7.0, device=DEV), torch.full((D,), 7.0, device=DEV)
    ops.obs_norm_merge(state, dev(stats, torch.float64), (1 << D) - 1 if mask is None else mask, eps, mu, inv)
    return state.cpu().numpy(), mu.cpu().numpy(), inv.cpu().numpy()


@pytest.mark.parametrize("D", [6, 7, 8])
def test_merge_three_batches_against_merge_running(ops, D):
    from uavppo.obs_norm import batch_stats, merge_running
    rng = np.random.default_rng(20 + D)
    state, ref = torch.zeros(2 + 2 * D, dtype=torch.float64, device=DEV), np.zeros(2 + 2 * D)
    for rows in (40, 333, 7):
        st = batch_stats(_obs(rng, rows, D))
        got = _merge(ops, state, st, D)
        ref, mu, inv = merge_running(ref, st, 1e-4)
        _merge_close(*got, ref, mu, inv)
    assert ref[0] == 380.0 and ref[1] == 0.0 and inv[2] < 0.05


def test_merge_edge_cases(ops):
    from uavppo.obs_norm import batch_stats, merge_running
    D, f64 = 6, dict(dtype=torch.float64, device=DEV)
    rng = np.random.default_rng(9)
    # an empty state and a batch that is skipped (a NaN in one channel's sum): the identity, one skip, nothing else moves
    bad = batch_stats(_obs(rng, 20, D))
    bad[1 + 4] = np.nan
    state, mu, inv = _merge(ops, torch.zeros(14, **f64), bad, D)
    assert state.tolist() == [0.0, 1.0] + [0.0] * 12 and np.all(mu == 0.0) and np.all(inv == 1.0)
    # a zero-variance channel: inv_sigma = 1 / sqrt(eps) = 100
    x = _obs(rng, 27, D)
    x[:, 5] = 0.25
    state_t = torch.zeros(14, **f64)
    state, mu, inv = _merge(ops, state_t, batch_stats(x), D)
    ref = merge_running(np.zeros(14), batch_stats(x), 1e-4)
    _merge_close(state, mu, inv, *ref)
    assert state[2 + 5] == 0.25 and state[2 + D + 5] == 0.0 and mu[5] == np.float32(0.25) and _ulps(inv[5:6], np.float32([100.0])) <= 1
    # a running estimate survives non-finite batches whole: every channel as it was, skipped counted, mu / inv_sigma restated
    before = state.copy()
    for k, (slot, v) in enumerate(((1 + 2, np.nan), (1 + D + 3, np.inf), (1, -np.inf))):
        bad = batch_stats(_obs(rng, 20, D))
        bad[slot] = v
        after, mu2, inv2 = _merge(ops, state_t, bad, D)
        assert np.array_equal(np.delete(after, 1), np.delete(before, 1)) and after[1] == k + 1.0
        assert np.array_equal(mu2, mu) and np.array_equal(inv2, inv)
    # a masked channel is tracked but passes as it is
    state, mu, inv = _merge(ops, torch.zeros(14, **f64), batch_stats(x), D, mask=0b000100)
    assert np.all(state[2:8] != 0.0) and mu[2] != 0.0 and inv[2] < 0.05
    assert np.all(np.delete(mu, 2) == 0.0) and np.all(np.delete(inv, 2) == 1.0)


# ------------------------------------------------------------------------------------------------ 3: fold, unfold_grad, unfold
def _first_layer(rows, D):
    rng = np.random.default_rng(rows + D)
    w = (rng.standard_normal((rows, D)) * 0.1).astype(np.float32)
    b = (rng.standard_normal(rows) * 0.1).astype(np.float32)
    mu = rng.standard_normal(D).astype(np.float32)
    inv = (1.0 / (0.2 + rng.random(D) * 30.0)).astype(np.float32)
    mu[2], inv[2], inv[5] = 37.5, 1.0 / 29.0, 100.0
    return rng, w, b, mu, inv


@pytest.mark.parametrize("rows,D", [(256, 6), (512, 8), (1024, 7)])       # 4H of h = 64 / 128 / 256; the MLP's h1
def test_fold_unfold_grad_and_unfold_against_numpy(ops, rows, D):
    from uavppo import obs_norm as on
    rng, w, b, mu, inv = _first_layer(rows, D)
    tw, tb, tmu, tinv = dev(w), dev(b), dev(mu), dev(inv)
    w_eff, b_eff = torch.empty_like(tw), torch.empty_like(tb)
    want_w, want_b = on.fold(w, b, mu, inv)
    for start in (0.0, 1e6):                                              # pmax is raised, never lowered
        pmax = torch.full((1,), start, device=DEV)
        ops.obs_fold(tw, tb, tmu, tinv, w_eff, b_eff, pmax)
        true_max = max(w_eff.abs().max().item(), b_eff.abs().max().item())
        assert 1.0 < true_max < 1e6 and pmax.item() == max(start, true_max)
    assert _ulps(w_eff.cpu().numpy(), want_w) <= 1 and _ulps(b_eff.cpu().numpy(), want_b) <= 1
    assert np.array_equal(_bits(tw), w.view(np.uint32)) and np.array_equal(_bits(tb), b.view(np.uint32))
    ops.obs_fold(tw, tb, tmu, tinv, w_eff, b_eff)                         # without a pmax slot
    # identity statistics: bit for bit
    wi, bi = torch.empty_like(tw), torch.empty_like(tb)
    ops.obs_fold(tw, tb, torch.zeros(D, device=DEV), torch.ones(D, device=DEV), wi, bi)
    assert np.array_equal(_bits(wi), w.view(np.uint32)) and np.array_equal(_bits(bi), b.view(np.uint32))
    # the gradient back, in place; db stays
    gw, gb = rng.standard_normal((rows, D)).astype(np.float32), rng.standard_normal(rows).astype(np.float32)
    tgw, tgb = dev(gw), dev(gb)
    ops.obs_unfold_grad(tgw, tgb, tmu, tinv)
    assert _ulps(tgw.cpu().numpy(), on.unfold_grad(gw, gb, mu, inv)) <= 1
    assert np.array_equal(_bits(tgb), gb.view(np.uint32))
    # the parameters back: into other arrays, and in place
    w2, b2 = torch.empty_like(tw), torch.empty_like(tb)
    ops.obs_unfold(w_eff, b_eff, tmu, tinv, w2, b2)
    ref_w, ref_b = on.unfold(w_eff.cpu().numpy(), b_eff.cpu().numpy(), mu, inv)
    assert _ulps(w2.cpu().numpy(), ref_w) <= 1 and _ulps(b2.cpu().numpy(), ref_b) <= 1
    assert np.abs(w2.cpu().numpy() - w).max() <= 3 * 2.0 ** -24 * np.abs(w).max()
    ops.obs_unfold(w_eff, b_eff, tmu, tinv, w_eff, b_eff)
    assert np.array_equal(_bits(w_eff), _bits(w2)) and np.array_equal(_bits(b_eff), _bits(b2))


def test_the_calls_refuse_what_the_header_says_they_refuse(ops):
    from uavppo import _lib
    lib, h = _lib.lib(), ops.Context.get(torch.device(DEV)).handle
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    f32, f64 = dict(dtype=torch.float32, device=DEV), dict(dtype=torch.float64, device=DEV)
    obs, stats, state = torch.ones(4, 8, **f32), torch.zeros(17, **f64), torch.zeros(18, **f64)
    w, b, mu, inv = torch.ones(4, 8, **f32), torch.ones(4, **f32), torch.zeros(8, **f32), torch.ones(8, **f32)
    P = lambda t: C.c_void_p(t.data_ptr())
    refused = [
        lib.uav_obs_stats(h, P(obs), 4, 5, 8, P(stats), s), lib.uav_obs_stats(h, P(obs), 4, 9, 9, P(stats), s),
        lib.uav_obs_stats(h, P(obs), 0, 8, 8, P(stats), s), lib.uav_obs_stats(h, P(obs), 4, 8, 7, P(stats), s),
        lib.uav_obs_stats(h, None, 4, 8, 8, P(stats), s), lib.uav_obs_stats(h, P(obs), 4, 8, 8, None, s),
        lib.uav_obs_stats(None, P(obs), 4, 8, 8, P(stats), s),
        lib.uav_obs_norm_merge(h, P(state), P(stats), 8, 0xFF, 0.0, P(mu), P(inv), s),
        lib.uav_obs_norm_merge(h, P(state), P(stats), 8, 0xFF, -1e-4, P(mu), P(inv), s),
        lib.uav_obs_norm_merge(h, P(state), P(stats), 8, 0xFF, float("nan"), P(mu), P(inv), s),
        lib.uav_obs_norm_merge(h, P(state), P(stats), 5, 0xFF, 1e-4, P(mu), P(inv), s),
        lib.uav_obs_norm_merge(h, None, P(stats), 8, 0xFF, 1e-4, P(mu), P(inv), s),
        lib.uav_obs_norm_merge(h, P(state), P(stats), 8, 0xFF, 1e-4, None, P(inv), s),
        lib.uav_obs_fold(h, P(w), P(b), 4, 9, P(mu), P(inv), P(w), P(b), None, s),
        lib.uav_obs_fold(h, P(w), P(b), 0, 8, P(mu), P(inv), P(w), P(b), None, s),
        lib.uav_obs_fold(h, P(w), None, 4, 8, P(mu), P(inv), P(w), P(b), None, s),
        lib.uav_obs_unfold_grad(h, P(w), P(b), 4, 5, P(mu), P(inv), s), lib.uav_obs_unfold_grad(h, P(w), P(b), -1, 8, P(mu), P(inv), s),
        lib.uav_obs_unfold_grad(h, None, P(b), 4, 8, P(mu), P(inv), s),
        lib.uav_obs_unfold(h, P(w), P(b), 4, 10, P(mu), P(inv), P(w), P(b), s), lib.uav_obs_unfold(h, P(w), P(b), 0, 8, P(mu), P(inv), P(w), P(b), s),
        lib.uav_obs_unfold(h, P(w), P(b), 4, 8, None, P(inv), P(w), P(b), s),
    ]
    assert refused == [2] * len(refused), refused
    assert b"uav_obs_unfold" in lib.uav_last_error()
    torch.cuda.synchronize()                                             # a refused call launches nothing
    assert stats.abs().max().item() == 0.0 and state.abs().max().item() == 0.0 and w.min().item() == 1.0 and mu.abs().max().item() == 0.0


# ------------------------------------------------------------------------------------------------ 4: trainer
CASES = [("mlp", 128, 1), ("lstm", 64, 1), ("lstm", 64, 2)]            # fused MLP; fused LSTM h = 64; a stacked LSTM (step-wise)


def _trainer(kind, hidden, layers=1, seed=3, cls=None, **kw):
    from uavppo.trainer import VecPPOTrainer
    kw = dict(dict(device=DEV, seed=seed, use_curriculum=False), **kw)
    return (cls or VecPPOTrainer)(8, 16, policy=kind, hidden=hidden, layers=layers, **kw)


def _first(tr, flat):
    """(w, b) of the first layer, as numpy, cut out of a flat parameter-sized vector."""
    on = tr.obs_norm
    n = on.rows * on.D
    f = flat.detach().cpu().numpy()
    return f[on._ow:on._ow + n].reshape(on.rows, on.D), f[on._ob:on._ob + on.rows]


def _assert_flat_is_the_fold_of_the_master(tr):
    from uavppo.obs_norm import fold
    on = tr.obs_norm
    w, b = _first(tr, on.master)
    w_eff, b_eff = _first(tr, tr.policy.flat)
    want_w, want_b = fold(w, b, on.mu.cpu().numpy(), on.inv_sigma.cpu().numpy())
    assert _ulps(w_eff, want_w) <= 1 and _ulps(b_eff, want_b) <= 1
    rest = torch.ones_like(on.master, dtype=torch.bool)
    rest[on._ow:on._ow + on.rows * on.D] = False
    rest[on._ob:on._ob + on.rows] = False
    assert torch.equal(tr.policy.flat[rest].view(torch.int32), on.master[rest].view(torch.int32))


def _oracle_gradient(tr, params_flat, obs64):
    """f64 gradient of the PPO loss the update just took a step on (tr.adv_n / tr.ret, one minibatch) at the parameters
    `params_flat`, of the policy applied to `obs64` [N][T][D] (f64): the oracle's forward and loss, autograd in f64."""
    from _iteration_check import named_from_flat, oracle_gradient_chunked
    from oracle import ppo_oracle as po
    p = {k: v.double() for k, v in named_from_flat(tr.policy, params_flat.detach().cpu()).items()}
    b = {k: v.detach().cpu() for k, v in tr.buf.items()}
    if tr.kind == "lstm":
        buf = dict(b, obs=torch.as_tensor(obs64))
        return oracle_gradient_chunked(p, buf, tr.h0, tr.c0, tr.adv_n, tr.ret)["grad"]
    leaf = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    probs, value, _ = po.mlp_forward(leaf, torch.as_tensor(obs64).reshape(-1, obs64.shape[-1]))
    total = po.ppo_losses(probs, value.reshape(-1), b["act"].reshape(-1).long(), b["logp"].reshape(-1).double(),
                          tr.adv_n.cpu().reshape(-1).double(), tr.ret.cpu().reshape(-1).double(), b["val"].reshape(-1).double())[0]
    names = list(leaf)
    return dict(zip(names, torch.autograd.grad(total, [leaf[k] for k in names])))


def _gradient_error(kind, hidden, layers, on):
    """Relative L2 error of the first optimiser step's (master) gradient of the second iteration against the f64 oracle."""
    from _iteration_check import grad_errors, named_from_flat
    tr = _trainer(kind, hidden, layers, seed=11, normalise_obs=on, epochs=1)
    tr.train_iteration()                                   # with the option on: the statistics leave the identity here
    if on:                                                 # S_1: in force for the second rollout and all of its update
        mu, inv = tr.obs_norm.mu.cpu().numpy().astype(np.float64), tr.obs_norm.inv_sigma.cpu().numpy().astype(np.float64)
        assert np.abs(inv - 1.0).min() > 0.5                # every channel is away from the identity
    tr.collect()
    tr.record_grads = True
    tr.update()
    g, p = tr.grad_log[0]
    obs = tr.buf["obs"].cpu().numpy().astype(np.float64)
    if on:
        obs = (obs - mu) * inv
    want = _oracle_gradient(tr, p, obs)
    got = named_from_flat(tr.policy, g.cpu())
    per, rel = grad_errors(got, want)
    return rel, max(per.values())


# The multiple of the un-normalised trainer's own error (the yardstick: the same trainer without the option against the same
# oracle on raw observations) the fold path is allowed.  Two things the fold adds to the kernels' f32 error: (1) w_eff and b_eff
# are each one more f32 rounding of the parameters the gradient is taken at (2^-24 relative on every first-layer weight, and on
# b_eff one rounding at the size of sum_j |w_eff_j mu_j|, which exceeds |b|); (2) dw = (dw_eff - db mu) / sigma subtracts two
# f32 gradients that agree in their leading digits wherever a channel moves little against its mean -- for a channel that is
# constant so far (o[5] with the curriculum off) they cancel completely and the rounding left over is multiplied by
# 1 / sqrt(eps) = 100.  Measured on one MI355X at these shapes (profiles/obs_norm_accuracy.json; relative L2, un-normalised ->
# fold path): fused MLP 7.7e-07 -> 3.2e-07 (x 0.41), LSTM h = 64 1.2e-07 -> 2.1e-07 (x 1.76), stacked LSTM 2.1e-07 -> 2.3e-07
# (x 1.13), with inv_sigma between 3 and 91 in force.  The margin is twice the largest ratio seen, rounded up.
GRAD_MARGIN = 4.0


@pytest.mark.parametrize("kind,hidden,layers", CASES)
def test_the_gradient_is_the_gradient_of_the_normalised_policy(kind, hidden, layers):
    base, base_worst = _gradient_error(kind, hidden, layers, on=False)
    fold, fold_worst = _gradient_error(kind, hidden, layers, on=True)
    print(f"[obs_norm accuracy] {kind} h={hidden} L={layers}: rel L2 of the gradient against f64: un-normalised {base:.3e} "
          f"(worst tensor {base_worst:.3e}), fold path {fold:.3e} (worst tensor {fold_worst:.3e}), ratio {fold / base:.2f}")
    assert fold <= GRAD_MARGIN * base, (fold, base)


# approx_kl (the k3 estimator) and the k1 estimator of the first step: what the un-normalised trainer meets at these shapes, measured
# (one MI355X, all three cases): both sums are exactly 0 -- the update's first forward pass reproduces the rollout's log-probabilities
# to the bit -- and so they are with the option on.  The test asserts it of both trainers.
FIRST_STEP_KL = 0.0


@pytest.mark.parametrize("kind,hidden,layers", CASES)
def test_the_ratio_is_one_at_the_first_step(kind, hidden, layers):
    seen = {}
    for on in (False, True):
        tr = _trainer(kind, hidden, layers, seed=12, normalise_obs=on, epochs=1, diagnostics=True)
        tr.train_iteration()
        tr.train_iteration()                               # on: rollout and update on S_1, not the identity
        d = tr.diagnostics()
        seen[on] = (d["approx_kl"][0], d["approx_kl_k1"][0], d["clip_fraction"][0])
        if on:
            assert (tr.obs_norm.inv_sigma - 1.0).abs().min().item() > 0.5      # away from the identity
    print(f"[obs_norm first step] {kind} h={hidden} L={layers}: (k3, k1, clip fraction) un-normalised {seen[False]}, fold path {seen[True]}")
    for on in (False, True):
        assert abs(seen[on][0]) <= FIRST_STEP_KL and abs(seen[on][1]) <= FIRST_STEP_KL and seen[on][2] == 0.0, (on, seen[on])


class _CountingLib:
    """The C ABI behind a proxy that counts the calls of every entry point."""

    def __init__(self, lib):
        self._lib, self.calls = lib, {}

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("uav_"):
            return fn

        def counted(*a):
            self.calls[name] = self.calls.get(name, 0) + 1
            return fn(*a)
        return counted


def _counted_iterations(monkeypatch, n, **kw):
    from uavppo import _lib, ops
    proxy = _CountingLib(_lib.lib())
    tr = _trainer(**kw)
    monkeypatch.setattr(ops, "lib", lambda: proxy)
    for _ in range(n):
        tr.train_iteration()
    torch.cuda.synchronize()
    monkeypatch.undo()
    return tr, proxy.calls


@pytest.mark.parametrize("kind,hidden", [("mlp", 128), ("lstm", 64)])
def test_option_off_is_the_trainer_without_the_keyword(kind, hidden, monkeypatch):
    """Byte-identical parameters and moments after seeded iterations, and the same entry points called the same number of times;
    with the option on: two more calls per optimiser step and three per iteration (uav_obs_stats, merge, fold)."""
    a, calls_a = _counted_iterations(monkeypatch, 3, kind=kind, hidden=hidden, seed=4)
    b, calls_b = _counted_iterations(monkeypatch, 3, kind=kind, hidden=hidden, seed=4, normalise_obs=False)
    assert b.obs_norm is None and calls_a == calls_b and not any(k.startswith("uav_obs_") for k in calls_b)
    assert torch.equal(a.policy.flat.view(torch.int32), b.policy.flat.view(torch.int32))
    assert torch.equal(a.exp_avg_sq.view(torch.int32), b.exp_avg_sq.view(torch.int32))
    c, calls_c = _counted_iterations(monkeypatch, 3, kind=kind, hidden=hidden, seed=4, normalise_obs=True)
    steps = c.opt_step
    extra = {k: v - calls_a.get(k, 0) for k, v in calls_c.items() if v != calls_a.get(k, 0)}
    assert steps == 3 * c.hp["epochs"]
    assert extra == {"uav_obs_unfold_grad": steps, "uav_obs_fold": steps + 3, "uav_obs_stats": 3, "uav_obs_norm_merge": 3}, extra
    assert not torch.equal(a.policy.flat, c.policy.flat)


@pytest.mark.parametrize("kind,hidden,layers,kw", [("mlp", 128, 1, {}), ("lstm", 64, 1, {}), ("lstm", 64, 2, {}), ("lstm", 256, 1, {}),
                                                   ("mlp", 128, 1, dict(trend_k=2, minibatch_rows=50)),
                                                   ("mlp", 128, 1, dict(fused_off=True)),
                                                   ("lstm", 64, 1, dict(num_minibatches=2, shuffle_envs=True, normalise_rewards=True)),
                                                   ("lstm", 64, 1, dict(bptt_len=8, target_kl=10.0, obs_norm_channels=(2,)))])
def test_the_statistics_follow_the_buffers_and_flat_is_the_fold_of_the_master(kind, hidden, layers, kw):
    """Over three iterations of every route: host_stats() is merge_running replayed over the buf["obs"] snapshots; policy.flat is
    the fold of the master behind every rollout and every update; buf["obs"] is never written."""
    from uavppo.obs_norm import batch_stats, merge_running
    kw = dict(kw)
    fused_off = kw.pop("fused_off", False)
    tr = _trainer(kind, hidden, layers, seed=5, normalise_obs=True, epochs=2, **kw)
    if fused_off:
        tr.fused_mlp = False                               # the layer-by-layer MLP route
    D, mask = tr.obs_dim, tr.obs_norm.mask
    ref = np.zeros(2 + 2 * D)
    hs = tr.obs_norm.host_stats()
    assert hs["count"] == 0.0 and np.all(hs["mu"] == 0.0) and np.all(hs["inv_sigma"] == 1.0)
    flat0 = tr.policy.flat.clone()
    for it in range(3):
        tr.collect()
        _assert_flat_is_the_fold_of_the_master(tr)
        snap = tr.buf["obs"].clone()
        tr.update()
        tr.iteration += 1
        assert torch.equal(tr.buf["obs"].view(torch.int32), snap.view(torch.int32))
        ref, mu, inv = merge_running(ref, batch_stats(snap.cpu().numpy().reshape(-1, D)), tr.obs_norm.eps, mask)
        hs = tr.obs_norm.host_stats()
        got_state = np.concatenate([[hs["count"], hs["skipped"]], hs["mean"], hs["var"] * hs["count"]])
        for g, r in zip(got_state, ref):
            assert abs(g - r) <= 1e-13 * abs(r) + 1e-300, (it, got_state, ref)      # var * count: one more f64 rounding than M2
        assert _ulps(hs["mu"], mu) <= 1 and _ulps(hs["inv_sigma"], inv) <= 1
        _assert_flat_is_the_fold_of_the_master(tr)
    tr.losses()                                            # raises on NaN
    assert hs["count"] == 3.0 * 8 * 16 and hs["skipped"] == 0.0 and abs(hs["inv_sigma"][2] - 1.0) > 0.5
    assert not torch.equal(flat0, tr.policy.flat)
    if kw.get("obs_norm_channels") == (2,):
        assert np.all(np.delete(hs["mu"], 2) == 0.0) and np.all(np.delete(hs["inv_sigma"], 2) == 1.0)


def test_freeze_stops_the_merge_and_reset_restores_the_identity(monkeypatch):
    from uavppo import _lib, ops
    tr = _trainer("mlp", 128, seed=6, normalise_obs=True, epochs=1)
    tr.train_iteration()
    before, master = tr.obs_norm.state.clone(), tr.obs_norm.master.clone()
    tr.obs_norm.freeze()
    proxy = _CountingLib(_lib.lib())
    monkeypatch.setattr(ops, "lib", lambda: proxy)
    tr.train_iteration()
    monkeypatch.undo()
    # frozen: the optimiser step's fold stands, nothing follows the update
    assert {k: v for k, v in proxy.calls.items() if k.startswith("uav_obs_")} == {"uav_obs_unfold_grad": 1, "uav_obs_fold": 1}
    assert torch.equal(tr.obs_norm.state, before) and not torch.equal(tr.obs_norm.master, master)       # Adam goes on
    _assert_flat_is_the_fold_of_the_master(tr)
    tr.obs_norm.unfreeze()
    tr.train_iteration()
    assert tr.obs_norm.state[0].item() == 2.0 * 8 * 16
    flat = tr.policy.flat.clone()
    tr.reset()
    hs = tr.obs_norm.host_stats()
    assert hs["count"] == 0.0 and np.all(hs["mu"] == 0.0) and np.all(hs["inv_sigma"] == 1.0)
    assert torch.equal(tr.policy.flat, flat) and torch.equal(tr.obs_norm.master, flat)      # the policy computes what it computed


def test_state_dict_round_trip_reproduces_the_next_iteration_bit_for_bit(tmp_path):
    from uavppo.obs_norm import save_state
    a = _trainer("mlp", 128, seed=7, normalise_obs=True, epochs=2)
    for _ in range(2):
        a.train_iteration()
    sd = a.obs_norm.state_dict()
    assert sorted(sd) == ["frozen", "inv_sigma", "master", "mu", "state"] and sd["state"].dtype == np.float64
    assert sd["master"].dtype == sd["mu"].dtype == sd["inv_sigma"].dtype == np.float32 and sd["mu"].shape == sd["inv_sigma"].shape == (6,)
    assert sd["state"].shape == (14,) and sd["state"][0] == 2.0 * 8 * 16 and sd["master"].shape == (a.policy.num_params(),)
    path = save_state(a.obs_norm, str(tmp_path / "policy.pth"))       # the run is continued from the file the scripts write
    b = _trainer("mlp", 128, seed=99, normalise_obs=True, epochs=2)
    b.obs_norm.load_state_dict(dict(np.load(path)))
    for x, y in ((b.obs_norm.state, a.obs_norm.state), (b.obs_norm.master, a.obs_norm.master), (b.obs_norm.mu, a.obs_norm.mu),
                 (b.obs_norm.inv_sigma, a.obs_norm.inv_sigma), (b.policy.flat, a.policy.flat)):
        assert np.array_equal(_bits(x), _bits(y))                         # policy.flat after the reload IS the saved model
    a.collect()
    for k in a.buf:
        b.buf[k].copy_(a.buf[k])
    b.exp_avg.copy_(a.exp_avg)
    b.exp_avg_sq.copy_(a.exp_avg_sq)
    b.opt_step = a.opt_step
    a.update()
    b.update()
    assert torch.equal(a.policy.flat.view(torch.int32), b.policy.flat.view(torch.int32))
    assert torch.equal(a.obs_norm.master.view(torch.int32), b.obs_norm.master.view(torch.int32))
    assert torch.equal(a.obs_norm.state, b.obs_norm.state)
    with pytest.raises(ValueError):
        b.obs_norm.load_state_dict(dict(sd, state=sd["state"][:5]))


@pytest.mark.parametrize("kind,hidden", [("mlp", 128), ("lstm", 64)])
def test_a_foreign_load_state_dict_re_derives_the_master(kind, hidden):
    from uavppo.obs_norm import unfold
    tr = _trainer(kind, hidden, seed=8, normalise_obs=True, epochs=1)
    tr.train_iteration()
    on = tr.obs_norm
    mu, inv = on.mu.cpu().numpy().copy(), on.inv_sigma.cpu().numpy().copy()       # S_1, in force until the next update ends
    assert np.abs(inv - 1.0).min() > 0.5
    other = _trainer(kind, hidden, seed=31).policy.state_dict()
    tr.policy.load_state_dict(other)                       # folded, deployable parameters, written behind the normaliser's back
    loaded = tr.policy.flat.clone()
    tr.collect()
    assert torch.equal(tr.policy.flat.view(torch.int32), loaded.view(torch.int32))      # the rollout ran on what was loaded
    tr.record_grads = True
    tr.update()
    master_at_step_0 = tr.grad_log[0][1]
    w, b = _first(tr, master_at_step_0)
    want_w, want_b = unfold(*_first(tr, loaded), mu, inv)
    assert _ulps(w, want_w) <= 1 and _ulps(b, want_b) <= 1 and not np.array_equal(w, _first(tr, loaded)[0])
    rest = torch.ones_like(loaded, dtype=torch.bool)
    rest[on._ow:on._ow + on.rows * on.D] = False
    rest[on._ob:on._ob + on.rows] = False
    assert torch.equal(master_at_step_0[rest].view(torch.int32), loaded[rest].view(torch.int32))
    _assert_flat_is_the_fold_of_the_master(tr)


_CHILD = """
import hashlib, json, sys
sys.path[:0] = [%r, %r]
import torch
from uavppo.dist_utils import collectives_on, use_abi_collectives
from uavppo.trainer import VecPPOTrainer
use_abi_collectives(0, 1, "cuda:0")
assert collectives_on()
tr = VecPPOTrainer(8, 16, policy="lstm", hidden=64, device="cuda:0", seed=8, normalise_obs=True)
for _ in range(2):
    tr.train_iteration()
tr.losses()
sha = lambda t: hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()
print(json.dumps({"flat": sha(tr.policy.flat), "master": sha(tr.obs_norm.master), "state": tr.obs_norm.state.cpu().tolist()}))
"""


def test_the_all_reduce_of_the_batch_sums_on_a_one_rank_communicator_changes_nothing():
    """The normaliser's exchange issued for real: a one-rank RCCL communicator on the C ABI's carrier with UAVPPO_FORCE_COLLECTIVES=1
    (the carrier is process-wide state, hence a child process), against the same job here, without collectives."""
    import hashlib
    import subprocess
    import sys
    from uavppo.trainer import VecPPOTrainer
    code = _CHILD % (ROOT, os.path.join(ROOT, "uav-wrf-les-ppo-lstm_amd"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120, env=dict(os.environ, UAVPPO_FORCE_COLLECTIVES="1"))
    assert r.returncode == 0, r.stderr[-2000:]
    abi = json.loads(r.stdout.strip().splitlines()[-1])
    tr = VecPPOTrainer(8, 16, policy="lstm", hidden=64, device=DEV, seed=8, normalise_obs=True)
    for _ in range(2):
        tr.train_iteration()
    tr.losses()
    sha = lambda t: hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()
    plain = {"flat": sha(tr.policy.flat), "master": sha(tr.obs_norm.master), "state": tr.obs_norm.state.cpu().tolist()}
    assert plain == abi and plain["state"][0] == 2.0 * 8 * 16


def test_gail_runs_normalised_and_its_discriminator_reads_the_raw_buffer(ops):
    from uavppo.gail import GAILTrainer
    rng = np.random.RandomState(31)
    expert = (rng.rand(200, 6).astype(np.float32), rng.randint(0, 5, 200).astype(np.int64))
    tr = _trainer("mlp", 128, seed=5, cls=GAILTrainer, expert=expert, gail_coef=0.5, env_coef=0.75, normalise_obs=True)
    for _ in range(2):
        tr.collect()
        obs0 = tr.buf["obs"].clone()
        tr.update()
        assert tr._rows()[0].data_ptr() == tr.buf["obs"].data_ptr()
        shaped = ops.disc_reward(tr.disc.flat, obs0.view(8 * 16, 6), tr.buf["act"].view(-1), tr.n_act, 0.5, 0.75,
                                 rew_env=tr.buf["rew"].view(-1)).view(8, 16)
        assert torch.equal(tr.rew_shaped.view(torch.int32), shaped.view(torch.int32))
        tr._after_update()
        assert torch.equal(tr.buf["obs"].view(torch.int32), obs0.view(torch.int32))
        tr.iteration += 1
    tr.losses()
    assert tr.obs_norm.state[0].item() == 2.0 * 8 * 16 and abs(tr.obs_norm.inv_sigma[2].item() - 1.0) > 0.5
    _assert_flat_is_the_fold_of_the_master(tr)


@pytest.mark.parametrize("kind,hidden", [("mlp", 128), ("lstm", 64)])
def test_the_saved_model_evaluates_unchanged(kind, hidden, tmp_path):
    """policy.state_dict() is the folded model: saved, loaded into a fresh policy that knows nothing of the normaliser, it gives
    under evaluate() the training policy's results; obs_norm_state.npz lands beside it."""
    import evaluate_with_lstm as ev
    from uavppo.obs_norm import STATE_FILE, save_state
    from uavppo.policy import LSTMActorCritic, MLPActorCritic
    from uavppo.vec_env import VecMethaneEnv
    tr = _trainer(kind, hidden, seed=9, normalise_obs=True, epochs=1)
    for _ in range(2):
        tr.train_iteration()
    path = str(tmp_path / "model" / "policy.pth")
    os.makedirs(os.path.dirname(path))
    torch.save(tr.policy.state_dict(), path)
    assert save_state(tr.obs_norm, path) == os.path.join(os.path.dirname(path), STATE_FILE)
    z = np.load(os.path.join(os.path.dirname(path), STATE_FILE))
    assert z["state"][0] == 2.0 * 8 * 16 and z["eps"] == 1e-4 and z["mask"] == 63 and z["master"].shape == (tr.policy.num_params(),)
    fresh = LSTMActorCritic(6, hidden, 1, 5, DEV, seed=77) if kind == "lstm" else MLPActorCritic(6, 5, device=DEV, seed=77)
    fresh.load_state_dict(torch.load(path, map_location="cpu"))
    assert torch.equal(fresh.flat.view(torch.int32), tr.policy.flat.view(torch.int32))
    res = [ev.evaluate(p, VecMethaneEnv(16, "v2.0", DEV, seed=3), max_steps=40) for p in (tr.policy, fresh)]
    for k in res[0]:
        assert np.array_equal(res[0][k], res[1][k]), k
