"""Running observation normalisation folded into the first layer, the host side: the option's surface (defaults off, the ctypes
rows, keyword validation) and the numpy functions of uavppo/obs_norm.py that state the kernels' definitions -- batch_stats
against math.fsum, merge_running against a two-pass evaluation of the concatenated batches, fold / unfold / unfold_grad against
plain f64 algebra.  No GPU."""
import inspect
import math
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "uavppo.h")


def _obs(rng, rows, D):
    """Observations as the environment scales them: O(1) channels, o[2] in [0, 100] with both ends present."""
    x = rng.standard_normal((rows, D)).astype(np.float32)
    x[:, 2] = (rng.random(rows) * 100.0).astype(np.float32)
    x[0, 2] = 0.0
    x[-1, 2] = 100.0
    return x


# ------------------------------------------------------------------------------------------------ 1: surface
def test_the_option_is_off_by_default():
    import config
    from uavppo.gail import GAILTrainer
    from uavppo.trainer import VecPPOTrainer
    assert config.NORMALISE_OBS is False and config.OBS_NORM_EPS == 1e-4
    p = inspect.signature(VecPPOTrainer.__init__).parameters
    assert p["normalise_obs"].default is False and p["obs_norm_eps"].default == 1e-4 and p["obs_norm_channels"].default is None
    g = inspect.signature(GAILTrainer.__init__).parameters
    assert "normalise_obs" not in g and g["kw"].kind is inspect.Parameter.VAR_KEYWORD      # inherited through **kw


def test_ctypes_rows_have_the_headers_argument_counts():
    from uavppo import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name, count in (("uav_obs_stats", 7), ("uav_obs_norm_merge", 9), ("uav_obs_fold", 11), ("uav_obs_unfold_grad", 8),
                        ("uav_obs_unfold", 10)):
        m = re.search(r"\b%s\s*\((.*?)\)\s*;" % name, src, flags=re.S)
        assert m, name
        assert len(m.group(1).split(",")) == count == len(_lib.SIGNATURES[name][1]), name
        assert hasattr(_lib.lib(), name)


@pytest.mark.parametrize("kw", [dict(normalise_obs=1), dict(normalise_obs="yes"), dict(normalise_obs=None), dict(obs_norm_eps=0.0),
                                dict(obs_norm_eps=-1e-4), dict(obs_norm_eps=float("inf")), dict(obs_norm_eps=float("nan")),
                                dict(obs_norm_eps="1e-4"), dict(obs_norm_eps=True), dict(obs_norm_channels=2), dict(obs_norm_channels="2"),
                                dict(obs_norm_channels=[6]), dict(obs_norm_channels=[-1]), dict(obs_norm_channels=[1.0]),
                                dict(obs_norm_channels=[True])])
def test_keyword_validation_raises_before_anything_is_allocated(kw):
    """ValueError, not the RuntimeError of a missing GPU: the check runs before the trainer touches a device -- with the option
    off as well (a bad value is refused wherever it is given)."""
    from uavppo.trainer import VecPPOTrainer
    for on in (True, False):
        with pytest.raises(ValueError):
            VecPPOTrainer(8, 16, policy="mlp", **dict(dict(normalise_obs=on), **kw))


def test_keyword_validation_accepts_what_the_issue_allows():
    from uavppo.obs_norm import check_obs_norm
    assert check_obs_norm(False, 1e-4, None, 6) == (False, 1e-4, 0b111111)
    assert check_obs_norm(True, 1, None, 8) == (True, 1.0, 0xFF)
    assert check_obs_norm(True, np.float32(0.5), (2, 6, 7), 8) == (True, 0.5, 0b11000100)
    assert check_obs_norm(np.bool_(True), 1e-8, iter([2, 2]), 7) == (True, 1e-8, 0b100)
    assert check_obs_norm(True, 1e-4, [], 6)[2] == 0
    with pytest.raises(ValueError):
        check_obs_norm(True, 1e-4, None, 9)            # more channels than the fold kernels take
    assert check_obs_norm(False, 1e-4, None, 9)[0] is False


# ------------------------------------------------------------------------------------------------ 2: the numpy statements
@pytest.mark.parametrize("rows,D", [(1, 6), (15, 7), (257, 8), (70001, 6)])
def test_batch_stats_is_an_f64_sum_in_a_fixed_order(rows, D):
    """Against math.fsum (the correctly rounded sum): any order of n non-negative f64 additions is within n * 2^-53 relative of
    it -- the squares -- and within n * 2^-53 * sum |x| absolutely for the signed sums."""
    from uavppo.obs_norm import batch_stats
    x = _obs(np.random.default_rng(rows), rows, D)
    st = batch_stats(x)
    assert st.shape == (1 + 2 * D,) and st.dtype == np.float64 and st[0] == rows
    x64 = x.astype(np.float64)
    for j in range(D):
        bar = rows * 2.0 ** -53
        assert abs(st[1 + j] - math.fsum(x64[:, j])) <= bar * math.fsum(np.abs(x64[:, j])) + 0.0
        q = math.fsum(x64[:, j] ** 2)
        assert abs(st[1 + D + j] - q) <= bar * q
    assert np.array_equal(batch_stats(x.reshape(1, rows, D)), st)          # [N][T][D] is its rows
    if rows <= 65536:                                                       # one row per slot: the order is the tree alone
        assert st[1 + 2] == batch_stats(x[:, 2:3].repeat(D, 1))[1]


def test_merge_of_three_batches_is_the_statistics_of_their_concatenation():
    from uavppo.obs_norm import batch_stats, merge_running
    rng = np.random.default_rng(5)
    D, eps = 8, 1e-4
    parts = [_obs(rng, n, D) for n in (40, 333, 7)]
    state = np.zeros(2 + 2 * D)
    for p in parts:
        state, mu, inv = merge_running(state, batch_stats(p), eps)
    x = np.concatenate(parts).astype(np.float64)
    mean, var = x.mean(0), x.var(0)
    assert state[0] == 380.0 and state[1] == 0.0
    # Chan's update is a handful of f64 operations per batch on values of the data's own size: 1e-12 relative is a wide bar for
    # three batches; the channel in [0, 100] has mean^2 / var of about 3, so the cancellation in q - s^2 / n costs one digit at most
    assert np.allclose(state[2:2 + D], mean, rtol=1e-12, atol=1e-13)
    assert np.allclose(state[2 + D:] / 380.0, var, rtol=1e-12)
    assert np.array_equal(mu, mean.astype(np.float32)) or np.abs(mu - mean).max() <= 1e-6 * np.abs(mean).max()
    assert np.allclose(inv, 1.0 / np.sqrt(var + eps), rtol=3e-7)
    assert inv[2] < 0.05 and inv[0] > 0.5          # the channel in [0, 100] is the one that is scaled down


def test_a_masked_channel_and_an_empty_state_stay_at_the_identity():
    from uavppo.obs_norm import batch_stats, merge_running
    rng = np.random.default_rng(6)
    x = _obs(rng, 50, 6)
    state, mu, inv = merge_running(np.zeros(14), batch_stats(x), 1e-4, mask=0b000100)
    assert state[0] == 50.0 and np.all(state[2:8] != 0.0)                   # every channel is tracked ...
    assert mu[2] != 0.0 and inv[2] != 1.0
    keep = [0, 1, 3, 4, 5]
    assert np.all(mu[keep] == 0.0) and np.all(inv[keep] == 1.0)             # ... and only the chosen one is applied
    # nothing merged yet (a batch without rows is a skipped batch): the identity for every channel
    state, mu, inv = merge_running(np.zeros(14), np.zeros(13), 1e-4)
    assert state.tolist() == [0.0, 1.0] + [0.0] * 12 and np.all(mu == 0.0) and np.all(inv == 1.0)
    # a constant channel: inv_sigma = 1 / sqrt(eps), the bound eps = 1e-4 is chosen for
    x[:, 5] = 0.25
    _, mu, inv = merge_running(np.zeros(14), batch_stats(x), 1e-4)
    assert mu[5] == np.float32(0.25) and inv[5] == np.float32(100.0)


def test_a_batch_with_a_nan_is_skipped_whole_and_counted():
    from uavppo.obs_norm import batch_stats, merge_running
    rng = np.random.default_rng(7)
    good, bad = _obs(rng, 30, 7), _obs(rng, 30, 7)
    bad[11, 4] = np.nan
    s0, mu0, inv0 = merge_running(np.zeros(16), batch_stats(good))
    s1, mu1, inv1 = merge_running(s0, batch_stats(bad))
    assert s1[1] == 1.0 and np.array_equal(np.delete(s1, 1), np.delete(s0, 1))          # every channel as it was, not only channel 4
    assert np.array_equal(mu1, mu0) and np.array_equal(inv1, inv0)
    bad[11, 4] = np.inf
    assert merge_running(s1, batch_stats(bad))[0][1] == 2.0


@pytest.mark.parametrize("rows,D", [(256, 6), (512, 8), (1024, 7)])
def test_fold_is_the_affine_map_of_the_normalised_observation_and_unfold_inverts_it(rows, D):
    from uavppo.obs_norm import fold, unfold, unfold_grad
    rng = np.random.default_rng(rows + D)
    w = (rng.standard_normal((rows, D)) * 0.1).astype(np.float32)
    b = (rng.standard_normal(rows) * 0.1).astype(np.float32)
    mu = rng.standard_normal(D).astype(np.float32)
    inv = (1.0 / (0.2 + rng.random(D) * 30.0)).astype(np.float32)
    mu[2], inv[2] = 37.5, 1.0 / 29.0
    w_eff, b_eff = fold(w, b, mu, inv)
    assert w_eff.dtype == b_eff.dtype == np.float32
    x = _obs(rng, 20, D).astype(np.float64)
    want = ((x - mu) * inv.astype(np.float64)) @ w.astype(np.float64).T + b
    got = x @ w_eff.astype(np.float64).T + b_eff
    # two f32 roundings (w_eff, b_eff) of terms up to max |w x^| ~ 0.1 * 100 / 29 * ... : 1e-5 absolute is 30 ulp of the largest
    assert np.abs(got - want).max() <= 1e-5
    # identity statistics: bit for bit
    wi, bi = fold(w, b, np.zeros(D, np.float32), np.ones(D, np.float32))
    assert np.array_equal(wi.view(np.uint32), w.view(np.uint32)) and np.array_equal(bi.view(np.uint32), b.view(np.uint32))
    # unfold(fold(w, b)) = (w, b) to f32 rounding: w through one product and one quotient (<= 1 ulp each, 2 together, plus the
    # rounding of the stored value: 3 ulp of f32 is the bar); b through D products of size |w_eff mu| rounded once to f32 on
    # the way out and once on the way back
    w2, b2 = unfold(w_eff, b_eff, mu, inv)
    assert np.abs(w2 - w).max() <= 3 * 2.0 ** -24 * np.abs(w).max()
    assert np.abs(b2.astype(np.float64) - b).max() <= 2 * 2.0 ** -24 * (np.abs(b).max() + np.abs(w_eff * mu).sum(1).max())
    # the chain rule: d/dw and d/db of L(w_eff(w), b_eff(w, b)) for a linear L = <gw, w_eff> + <gb, b_eff>
    gw, gb = rng.standard_normal((rows, D)).astype(np.float32), rng.standard_normal(rows).astype(np.float32)
    dw = unfold_grad(gw, gb, mu, inv)
    want_dw = (gw.astype(np.float64) - gb.astype(np.float64)[:, None] * mu) * inv
    assert dw.dtype == np.float32 and np.abs(dw - want_dw).max() <= 2.0 ** -24 * np.abs(want_dw).max()
    h = 1e-3                                              # L is linear in w: a finite difference is exact up to f32 rounding of the fold
    k, j = 3, 2
    wp = w.astype(np.float64).copy()
    wp[k, j] += h
    weff_p = wp * inv.astype(np.float64)
    L = lambda we, be: (gw.astype(np.float64) * we).sum() + (gb.astype(np.float64) * be).sum()
    L0 = L(w.astype(np.float64) * inv, b - (w.astype(np.float64) * inv * mu).sum(1))
    L1 = L(weff_p, b - (weff_p * mu).sum(1))
    assert abs((L1 - L0) / h - want_dw[k, j]) <= 1e-6 * max(1.0, abs(want_dw[k, j]))
