"""CPU: the host side of GAIL -- the reference's three names in model.py, the expert-pair cutter of generate_expert_data.py and
the shape answers of the discriminator entry points of the C ABI.  No compute call is made."""
import inspect

import numpy as np
import torch


def test_model_has_the_reference_gail_names_and_signatures():
    import model
    assert list(inspect.signature(model.Discriminator.__init__).parameters)[:3] == ["self", "state_dim", "action_dim"]
    for extra in ("device", "seed"):            # additive, with defaults: Discriminator(state_dim=6, action_dim=5) still works
        assert inspect.signature(model.Discriminator.__init__).parameters[extra].default is not inspect.Parameter.empty
    assert list(inspect.signature(model.compute_discriminator_loss).parameters) == [
        "discriminator", "expert_states", "expert_actions", "policy_states", "policy_actions"]
    sig = inspect.signature(model.get_expert_data)
    assert all(p.default is not inspect.Parameter.empty for p in sig.parameters.values())       # get_expert_data() as the reference calls it
    assert sig.parameters["path"].default == "expert_data.npz"
    # what train_ppo_gail.py imports first (train_ppo_gail.py:24-27)
    from model import PPOActorCritic, Discriminator, PPOTrainer, PPOBuffer, compute_discriminator_loss, get_expert_data  # noqa: F401
    import generate_expert_data
    import train_ppo_gail
    p = inspect.signature(generate_expert_data.generate_expert_data).parameters
    assert p["num_episodes"].default == 100 and p["out"].default == "expert_data.npz" and {"variant", "seed", "max_steps"} <= set(p)
    p = inspect.signature(train_ppo_gail.train_ppo_gail).parameters
    assert p["num_episodes"].default == 2000 and p["expert_path"].default == "expert_data.npz" and {"num_envs", "horizon"} <= set(p)
    from uavppo.gail import GAILTrainer
    from uavppo.trainer import VecPPOTrainer
    assert issubclass(GAILTrainer, VecPPOTrainer)
    p = inspect.signature(GAILTrainer.__init__).parameters
    assert p["disc_steps"].default == 1 and p["disc_lr"].default == 3e-5 and {"expert", "gail_coef", "env_coef"} <= set(p)


def test_get_expert_data_round_trips_the_reference_keys(tmp_path):
    import model
    rng = np.random.RandomState(0)
    states = rng.rand(37, 6)                    # the reference saves np.array(list of states): float64 unless the env says otherwise
    actions = rng.randint(0, 5, 37)
    path = str(tmp_path / "expert_data.npz")
    np.savez(path, states=states, actions=actions)
    s, a = model.get_expert_data(path)
    assert s.dtype == torch.float32 and tuple(s.shape) == (37, 6) and a.dtype == torch.int64 and tuple(a.shape) == (37,)
    assert np.array_equal(s.numpy(), states.astype(np.float32)) and np.array_equal(a.numpy(), actions)


def _loop_pairs(cur_obs0, obs_rec, act_rec, flags_rec):
    """generate_expert_data.py:35-51 env by env: state = what was acted on, appended with the action, until done."""
    S, A = [], []
    for n in range(len(cur_obs0)):
        state = cur_obs0[n]
        for t in range(obs_rec.shape[1]):
            if flags_rec[n, t] & 4:
                assert act_rec[n, t] == -1
                continue
            S.append(state)
            A.append(int(act_rec[n, t]))
            state = obs_rec[n, t]
    return np.array(S, dtype=np.float32).reshape(-1, cur_obs0.shape[1]), np.array(A, dtype=np.int64)


def _synthetic_records(lengths, steps, seed):
    """Records as uav_greedy_episodes leaves them: env n is stepped `lengths[n]` times (0 = never: it came in inactive), its last
    stepped slot carries the done bit (unless it ran into the end of the records), every later slot is 'not stepped'."""
    rng = np.random.RandomState(seed)
    N = len(lengths)
    cur = rng.rand(N, 6).astype(np.float32)
    obs = rng.rand(N, steps, 6).astype(np.float32)
    act = rng.randint(0, 5, (N, steps)).astype(np.int32)
    flags = np.zeros((N, steps), dtype=np.uint8)
    for n, L in enumerate(lengths):
        if 0 < L <= steps and not (L == steps and n % 2):      # odd envs of full length: cut off, no done bit
            flags[n, L - 1] = 1 | (2 if n % 3 == 0 else 0)
        flags[n, L:] = 4
        act[n, L:] = -1
        obs[n, L:] = 0.0
    return cur, obs, act, flags


def test_expert_pairs_equal_the_per_env_loop():
    from generate_expert_data import expert_pairs
    lengths = [5, 1, 0, 12, 7, 12, 3, 12]       # different lengths, one ending at step 0, one never stepped, full-length ones
    cur, obs, act, flags = _synthetic_records(lengths, 12, seed=1)
    want_s, want_a = _loop_pairs(cur, obs, act, flags)
    got_s, got_a = expert_pairs(cur, obs, act, flags)
    assert got_s.dtype == np.float32 and got_a.dtype == np.int64
    assert len(got_a) == sum(lengths) and np.array_equal(got_s, want_s) and np.array_equal(got_a, want_a)
    assert np.array_equal(got_s[0], cur[0]) and np.array_equal(got_s[5], cur[1])          # t = 0 acts on the reset observation
    # the terminal observation of env 0 (record 4) is never a state
    assert not (got_s == obs[0, 4]).all(1).any()
    # the same records arriving as two chunks (5 + 7 steps): env 3 / 5 / 7 span both, env 0 ends exactly at the cut
    parts = ([obs[:, :5], obs[:, 5:]], [act[:, :5], act[:, 5:]], [flags[:, :5], flags[:, 5:]])
    two_s, two_a = expert_pairs(cur, *parts)
    assert np.array_equal(two_s, want_s) and np.array_equal(two_a, want_a)
    # nobody stepped at all
    none_s, none_a = expert_pairs(*_synthetic_records([0, 0], 4, seed=2))
    assert none_s.shape == (0, 6) and none_a.shape == (0,)


def test_disc_param_count_and_shape_refusals_need_no_gpu():
    from uavppo import _lib
    lib = _lib.lib()
    assert lib.uav_disc_param_count(6, 5, 128) == 1665           # 128 * 11 + 128 + 128 + 1
    assert lib.uav_disc_param_count(8, 5, 128) == 128 * 13 + 257
    assert lib.uav_disc_param_count(10, 5, 128) == 128 * 15 + 257       # 10 + 5 + 1 = 16: the widest row that fits
    for od, na, h, word in ((11, 5, 128, b"obs_dim + n_act + 1 <= 16"), (6, 10, 128, b"obs_dim + n_act + 1 <= 16"),
                            (0, 5, 128, b"obs_dim=0"), (6, 5, 64, b"hidden=64"), (6, 5, 256, b"hidden=256")):
        assert lib.uav_disc_param_count(od, na, h) == 0 and word in lib.uav_last_error(), (od, na, h, lib.uav_last_error())
        # the compute entry points look at the shape before anything else: non-zero, with the reason, and no GPU touched
        rc = lib.uav_disc_grad(None, None, None, None, 1, None, None, 1, od, na, h, 1.0, 1.0, None, None, None)
        assert rc != 0 and b"uav_disc_grad" in lib.uav_last_error() and word in lib.uav_last_error()
        rc = lib.uav_disc_reward(None, None, None, None, 1, od, na, h, 1.0, 1.0, None, None, None)
        assert rc != 0 and b"uav_disc_reward" in lib.uav_last_error() and word in lib.uav_last_error()
    # a good shape gets past the shape check and is then refused for its NULL handle
    assert lib.uav_disc_grad(None, None, None, None, 1, None, None, 1, 6, 5, 128, 1.0, 1.0, None, None, None) != 0
    assert b"NULL" in lib.uav_last_error()
    from uavppo import ops
    assert ops.disc_param_count(6, 5) == 1665
    try:
        ops.disc_param_count(12, 5)
    except RuntimeError as e:
        assert "obs_dim + n_act + 1 <= 16" in str(e)
    else:
        raise AssertionError("ops.disc_param_count(12, 5) did not raise")


def test_as_action_index_accepts_indices_and_one_hot_rows():
    from uavppo.gail import as_action_index
    idx = torch.tensor([0, 4, 2, 2], dtype=torch.int64)
    assert as_action_index(idx, 5).dtype == torch.int32 and as_action_index(idx, 5).tolist() == [0, 4, 2, 2]
    hot = torch.zeros(4, 5)
    hot[range(4), idx] = 1.0
    hot[3] = 0.0                                 # a row with no action: no one-hot column
    assert as_action_index(hot, 5).tolist() == [0, 4, 2, -1]
    try:
        as_action_index(torch.full((2, 5), 0.2), 5)
    except RuntimeError as e:
        assert "one-hot" in str(e)
    else:
        raise AssertionError("soft action rows were accepted")
