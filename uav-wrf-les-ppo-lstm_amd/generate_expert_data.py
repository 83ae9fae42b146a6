# generate_expert_data.py -- expert (state, action) pairs for GAIL from greedy episodes of a trained policy.
#
# Counterpart of the reference's PPOV1.1/generate_expert_data.py: num_episodes greedy (argmax) episodes of a trained policy,
# every (state acted on, action) pair saved as expert_data.npz with the keys `states`, `actions` (:35-58).  The episodes run as
# that many PARALLEL environments through the evaluation path of evaluate_with_lstm.py: the fused greedy-episode kernels
# (uav_greedy_episodes) where they cover the policy (fused_refusal), the tail route (the LSTM layers' step kernels + uav_greedy_tail
# per env step) for every other LSTM policy (tail_refusal), the step-wise loop for what is left; all leave the same records
# (action, returned observation, flags per step), which expert_pairs() cuts into pairs on the host.
import numpy as np
import torch

from config import ENV_VARIANT, SEED
from evaluate_with_lstm import load_lstm_policy
from uavppo.greedy import GreedyRun, fused_refusal, policy_core, policy_route, stepwise_policy_probs  # noqa: F401  (fused_refusal: tests)
from uavppo.vec_env import VecMethaneEnv

NOT_STEPPED = 4          # bit 2 of a record's flags (include/uavppo.h, uav_greedy_episodes): the env was not stepped, act = -1


def expert_pairs(cur_obs0, obs_rec, act_rec, flags_rec):
    """(states f32 [M, obs_dim], actions i64 [M]) from the records of greedy episodes (host arrays).

    cur_obs0 [N, obs_dim]: the reset observations; obs_rec [N, S, obs_dim], act_rec [N, S], flags_rec [N, S]: per step the
    observation the step RETURNED, the action taken and the flags (bit0 done, bit1 reached, bit2 not stepped) -- or lists of
    such arrays, the chunks of successive launches, joined along the step axis.  The state of step t is the observation acted
    ON: the reset observation for t = 0, record t - 1 after that; slots flagged "not stepped" are dropped; episodes are
    concatenated in env order, steps in time order; the terminal observation is never a state
    (generate_expert_data.py:35-51)."""
    def join(x):
        return np.concatenate([np.asarray(c) for c in x], axis=1) if isinstance(x, (list, tuple)) else np.asarray(x)
    obs_rec, act_rec, flags_rec = join(obs_rec), join(act_rec), join(flags_rec)
    cur_obs0 = np.asarray(cur_obs0, dtype=np.float32)
    acted_on = np.concatenate([cur_obs0[:, None, :], obs_rec[:, :-1, :].astype(np.float32, copy=False)], axis=1)
    stepped = (flags_rec & NOT_STEPPED) == 0
    return np.ascontiguousarray(acted_on[stepped], dtype=np.float32), act_rec[stepped].astype(np.int64)


def expert_lengths(flags_rec):
    """Steps per episode, i64 [E], from the flags records expert_pairs takes (an array [N, S] or the list of the launches' chunks):
    the slots of env e that are not flagged "not stepped".  expert_pairs concatenates episodes in env order and steps in time
    order, so these lengths cut its flat arrays back into episodes (uavppo.bc.load_expert_sequences)."""
    flags_rec = np.concatenate([np.asarray(c) for c in flags_rec], axis=1) if isinstance(flags_rec, (list, tuple)) else np.asarray(flags_rec)
    return ((flags_rec & NOT_STEPPED) == 0).sum(axis=1).astype(np.int64)


def load_policy(path, device="cuda"):
    """A policy from a checkpoint train_ppo2.0.py writes: the LSTM actor-critic (keys lstm.*) or the reference's MLP
    (keys feature.*, model.PPOActorCritic; 6 inputs, or 6 + TREND_K read off feature.0.weight)."""
    sd = torch.load(path, map_location="cpu")
    if any(k.startswith("lstm.") for k in sd):
        return load_lstm_policy(path, device)
    from model import PPOActorCritic
    pol = PPOActorCritic(int(sd["feature.0.weight"].shape[1]), 5, device=device)
    pol.load_state_dict(sd)
    return pol


@torch.no_grad()
def greedy_records(policy, env, max_steps=None, chunk=250, fused=None, tail=None):
    """One greedy episode per environment of `env`: (reset observations [N, obs_dim], lists of per-chunk obs / act / flags
    records) as host arrays, in the record format of uav_greedy_episodes whichever path produced them.  fused / tail: as
    evaluate_with_lstm.evaluate (None: the fused kernels, else the tail route, else the step-wise loop)."""
    kind, core = policy_core(policy)
    N, dev = env.num_envs, env.device
    limit = max_steps or env.max_steps
    env.reset()
    cur_obs0 = env.obs.cpu().numpy().copy()
    obs_c, act_c, flags_c = [], [], []
    route = policy_route(policy, env, fused, tail, "greedy_records")
    run = GreedyRun(kind, core, env, tail=route == "tail") if route != "stepwise" else None
    if run is None:
        probs, nan = stepwise_policy_probs(kind, core, env)
        active, obs = torch.ones(N, dtype=torch.bool, device=dev), env.obs
    t0 = 0
    while t0 < limit:
        k = min(chunk, limit - t0)
        if run is not None:
            recs = run.chunk(t0, k)
            ro, ra, rf, active = recs["obs"], recs["act"], recs["flags"], run.active
        else:
            ro = torch.zeros(N, k, env.obs_dim, dtype=torch.float32, device=dev)
            ra = torch.full((N, k), -1, dtype=torch.int32, device=dev)
            rf = torch.full((N, k), NOT_STEPPED, dtype=torch.uint8, device=dev)
            for i in range(k):
                act = torch.argmax(probs(obs), dim=1).to(torch.int32)
                obs, _, done, _ = env.step(act)          # auto-reset: the env goes on, its later steps are not recorded
                done_b = done > 0.5
                ro[:, i] = torch.where(active[:, None], torch.where(done_b[:, None], env.term_obs, obs), ro[:, i])
                ra[:, i] = torch.where(active, act, ra[:, i])
                rf[:, i] = torch.where(active, env.flags & 3, rf[:, i])
                active = active & ~done_b
        obs_c.append(ro.cpu().numpy()), act_c.append(ra.cpu().numpy()), flags_c.append(rf.cpu().numpy())
        t0 += k
        if not bool(active.any()):
            break
    if run is not None:
        run.raise_on_nan()
    elif int(nan.item()) > 0:
        raise RuntimeError("NaN in probs")
    return cur_obs0, obs_c, act_c, flags_c


def generate_expert_data(policy="ppo_model.pth", num_episodes=100, variant=ENV_VARIANT, seed=SEED, max_steps=None,
                         out="expert_data.npz", device="cuda", fused=None, tail=None, lengths=False):
    """num_episodes greedy episodes of `policy` (an LSTMActorCritic, MLPActorCritic or model.PPOActorCritic, or the path of a
    checkpoint train_ppo2.0.py wrote; the reference loads 'ppo_model.pth') as num_episodes parallel environments seeded with
    `seed`; every (state, action) pair goes to `out` (None: not written).  Returns (states f32 [M, obs_dim], actions i64 [M]).
    The episodes run on the fused greedy kernels where they cover the policy, on the tail route (uav_greedy_tail behind the LSTM
    layers' step kernels) for every other LSTM policy, step-wise otherwise: the same pairs on each; fused / tail as
    evaluate_with_lstm.evaluate force a route.  lengths=True also saves the key `lengths` (expert_lengths: i64 [num_episodes],
    what behaviour cloning of an LSTM policy cuts the pairs into episodes with); the default writes the reference's two keys."""
    if isinstance(policy, (str, bytes)) or hasattr(policy, "__fspath__"):
        policy = load_policy(policy, device)
    _, core = policy_core(policy)
    trend_k = (core.obs_dim if hasattr(core, "obs_dim") else core.in_dim) - 6      # LSTMActorCritic | MLPActorCritic
    env = VecMethaneEnv(num_episodes, variant, core.device, seed=seed, trend_k=trend_k)
    recs = greedy_records(policy, env, max_steps, fused=fused, tail=tail)
    states, actions = expert_pairs(*recs)
    if out:
        extra = {"lengths": expert_lengths(recs[3])} if lengths else {}
        np.savez(out, states=states, actions=actions, **extra)
        print(f"expert data: {num_episodes} episodes, {len(actions)} pairs -> {out}")
    return states, actions


if __name__ == "__main__":
    generate_expert_data()
