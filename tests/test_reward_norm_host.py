"""Running return-based reward normalisation, the host side: the option's surface (defaults off, the ctypes rows, the ABI version,
keyword validation) and the two numpy functions of uavppo/reward_norm.py that state the kernels' definitions -- return_traces
against its own split, merge_running against a two-pass evaluation of the concatenated batches.  No GPU."""
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "uavppo.h")


def _rollout(rng, N, T, p_done=0.1):
    rew = rng.standard_normal((N, T)).astype(np.float32) * 3.0 + 0.5
    done = (rng.random((N, T)) < p_done).astype(np.float32)
    return rew, done


# ------------------------------------------------------------------------------------------------ 1: surface
def test_the_option_is_off_by_default():
    import config
    from uavppo.gail import GAILTrainer
    from uavppo.trainer import VecPPOTrainer
    assert config.NORMALISE_REWARDS is False and config.REWARD_CLIP == 10.0
    p = inspect.signature(VecPPOTrainer.__init__).parameters
    assert p["normalise_rewards"].default is False
    assert p["reward_clip"].default == 10.0
    assert p["reward_norm_gamma"].default is None
    g = inspect.signature(GAILTrainer.__init__).parameters
    assert "normalise_rewards" not in g and g["kw"].kind is inspect.Parameter.VAR_KEYWORD      # inherited through **kw


def test_ctypes_rows_have_the_headers_argument_counts_and_the_abi_version_stays():
    from uavppo import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name, count in (("uav_return_stats", 10), ("uav_return_norm_merge", 6), ("uav_reward_scale", 7)):
        m = re.search(r"\b%s\s*\((.*?)\)\s*;" % name, src, flags=re.S)
        assert m, name
        assert len(m.group(1).split(",")) == count == len(_lib.SIGNATURES[name][1]), name
    assert re.search(r"#define UAV_RETNORM_STATE_N 4\b", open(HEADER).read())
    assert re.search(r"#define UAV_ABI_VERSION 9\b", open(HEADER).read())
    assert _lib.lib().uav_abi_version() == 9


@pytest.mark.parametrize("kw", [dict(reward_clip=0.0), dict(reward_clip=-1.0), dict(reward_clip=float("inf")), dict(reward_clip=float("nan")),
                                dict(reward_clip="10"), dict(reward_clip=True), dict(reward_norm_gamma=-0.1), dict(reward_norm_gamma=1.5),
                                dict(reward_norm_gamma=float("nan")), dict(reward_norm_gamma="0.9")])
def test_keyword_validation_raises_before_anything_is_allocated(kw):
    """ValueError, not the RuntimeError of a missing GPU: the check runs before the trainer touches a device -- with the option
    off as well (a bad value is refused wherever it is given)."""
    from uavppo.trainer import VecPPOTrainer
    for on in (True, False):
        with pytest.raises(ValueError):
            VecPPOTrainer(8, 16, policy="mlp", normalise_rewards=on, **kw)


def test_keyword_validation_accepts_what_the_issue_allows():
    from uavppo.reward_norm import check_reward_norm
    assert check_reward_norm(10.0, None, 0.99) == (10.0, 0.99)
    assert check_reward_norm(None, 0.5, 0.99) == (0.0, 0.5)          # None: no clamp, 0.0 to the kernel
    assert check_reward_norm(np.float32(2.5), 0, 0.99) == (2.5, 0.0)
    assert check_reward_norm(1, 1, 0.99) == (1.0, 1.0)


def test_the_scripts_pass_the_config_names_and_save_the_state_beside_the_model(tmp_path):
    from types import SimpleNamespace
    from uavppo.reward_norm import STATE_FILE, save_state
    pkg = os.path.join(ROOT, "uav-wrf-les-ppo-lstm_amd")
    for script in ("train_ppo2.0.py", "train_ppo_gail.py"):
        src = open(os.path.join(pkg, script)).read()
        assert "normalise_rewards=NORMALISE_REWARDS, reward_clip=REWARD_CLIP" in src and "save_state(tr.reward_norm, model_path)" in src, script
    sd = {"state": np.array([1.0, 2.0, 3.0, 0.0]), "carry": np.arange(5.0)}
    fake = SimpleNamespace(gamma=0.99, clip=10.0, eps=1e-8, state_dict=lambda: sd)
    path = save_state(fake, str(tmp_path / "model" / "ppo.pth"))
    assert path == str(tmp_path / "model" / STATE_FILE) and STATE_FILE == "reward_norm_state.npz"
    got = np.load(path)
    assert sorted(got.files) == ["carry", "clip", "eps", "gamma", "state"]
    assert np.array_equal(got["state"], sd["state"]) and np.array_equal(got["carry"], sd["carry"]) and float(got["gamma"]) == 0.99


# ------------------------------------------------------------------------------------------------ 2: return_traces
@pytest.mark.parametrize("gamma", [0.99, 0.0, 1.0])
def test_return_traces_split_invariance_is_bitwise(gamma):
    from uavppo.reward_norm import return_traces
    rng = np.random.default_rng(3)
    N, T1, T2 = 5, 37, 64
    rew, done = _rollout(rng, N, T1 + T2)
    done[0, T1 - 1] = 1.0            # an episode that ends exactly at the cut
    done[1, T1] = 1.0                # ... and one that ends right behind it
    carry = rng.standard_normal(N)
    G, c = return_traces(rew, done, gamma, carry)
    G1, c1 = return_traces(rew[:, :T1], done[:, :T1], gamma, carry)
    G2, c2 = return_traces(rew[:, T1:], done[:, T1:], gamma, c1)
    assert np.array_equal(np.concatenate([G1, G2], 1), G) and np.array_equal(c2, c)
    assert c1[0] == 0.0 and c[0] == (0.0 if done[0, -1] else G[0, -1])


def test_return_traces_is_the_definition_on_a_row_worked_by_hand():
    from uavppo.reward_norm import return_traces
    G, c = return_traces([[1.0, 2.0, 3.0, 4.0]], [[0, 1, 0, 0]], 0.5, [8.0])
    assert G.tolist() == [[1.0 + 0.5 * 8.0, 2.0 + 0.5 * 5.0, 3.0, 4.0 + 0.5 * 3.0]] and c.tolist() == [5.5]
    G, c = return_traces([[1.0, 2.0]], [[0, 1]], 0.5, [0.0])
    assert c.tolist() == [0.0]


# ------------------------------------------------------------------------------------------------ 3: merge_running
def _two_pass(G):
    """{mean, M2, count} of all samples in one two-pass evaluation."""
    x = np.concatenate([np.asarray(g, dtype=np.float64).reshape(-1) for g in G])
    m = x.sum() / x.size
    return m, ((x - m) ** 2).sum(), float(x.size)


def _rel(a, b):
    return abs(a - b) / max(abs(b), 1e-300)


def test_merge_running_equals_the_two_pass_moments_of_the_concatenation():
    from uavppo.reward_norm import batch_stats, merge_running, return_traces
    rng = np.random.default_rng(11)
    state, carry, Gs, eps = np.zeros(4), np.zeros(6), [], 1e-8
    for T in (40, 64, 17):
        rew, done = _rollout(rng, 6, T)
        G, carry = return_traces(rew, done, 0.99, carry)
        Gs.append(G)
        state, scale = merge_running(state, batch_stats(G), eps)
    m, M2, n = _two_pass(Gs)
    assert _rel(state[0], m) <= 1e-12 and _rel(state[1], M2) <= 1e-12 and state[2] == n and state[3] == 0.0
    assert scale == np.float32(1.0 / np.sqrt(M2 / n + eps)) or abs(float(scale) - 1.0 / np.sqrt(M2 / n + eps)) <= 2.0 ** -23 * float(scale)
    assert scale.dtype == np.float32


def test_merging_the_summed_stats_of_two_env_shards_is_merging_the_unions():
    """The multi-rank claim: ranks all-reduce (sum) stats3 and each merges the total."""
    from uavppo.reward_norm import batch_stats, merge_running, return_traces
    rng = np.random.default_rng(12)
    s_union = s_sharded = np.zeros(4)
    carry = np.zeros(8)
    for _ in range(3):
        rew, done = _rollout(rng, 8, 33)
        G, carry = return_traces(rew, done, 0.99, carry)
        s_union, sc_u = merge_running(s_union, batch_stats(G))
        s_sharded, sc_s = merge_running(s_sharded, batch_stats(G[:3]) + batch_stats(G[3:]))
    assert all(_rel(a, b) <= 1e-12 for a, b in zip(s_sharded[:3], s_union[:3])) and s_sharded[2] == s_union[2]
    assert abs(float(sc_u) - float(sc_s)) <= 2.0 ** -23 * float(sc_u)


def test_a_batch_with_a_nan_leaves_the_state_and_counts_a_skip():
    from uavppo.reward_norm import batch_stats, merge_running, return_traces
    rng = np.random.default_rng(13)
    rew, done = _rollout(rng, 4, 20)
    G, _ = return_traces(rew, done, 0.99, np.zeros(4))
    state, scale = merge_running(np.zeros(4), batch_stats(G))
    bad = rew.copy()
    bad[2, 7] = np.nan
    Gb, _ = return_traces(bad, done, 0.99, np.zeros(4))
    with np.errstate(invalid="ignore"):
        after, scale2 = merge_running(state, batch_stats(Gb))
    assert np.array_equal(after[:3], state[:3]) and after[3] == 1.0 and scale2 == scale
    for s3 in ([np.inf, 1.0, 80.0], [1.0, np.inf, 80.0], [-np.inf, np.nan, 80.0]):
        after2, _ = merge_running(after, np.array(s3))
        assert np.array_equal(after2[:3], state[:3]) and after2[3] == 2.0


def test_a_constant_batch_and_an_empty_state_give_scale_one():
    from uavppo.reward_norm import batch_stats, merge_running
    state, scale = merge_running(np.zeros(4), batch_stats(np.full((3, 9), 2.5)))
    assert scale == np.float32(1.0) and state[1] == 0.0 and state[2] == 27.0 and state[0] == 2.5      # not 1 / sqrt(eps)
    with np.errstate(invalid="ignore"):
        state, scale = merge_running(np.zeros(4), np.array([np.nan, 1.0, 5.0]))                       # count stays 0
    assert scale == np.float32(1.0) and state.tolist() == [0.0, 0.0, 0.0, 1.0]
