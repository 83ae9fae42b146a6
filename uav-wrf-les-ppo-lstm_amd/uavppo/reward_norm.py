"""RewardNormaliser: reward scaling by a running estimate of the discounted return's standard deviation (the reward half of
"VecNormalize"), with no host read on the path.

Definitions (f64), per env row e of a rollout's rew / done [N][T]:
  trace   G[e][t] = rew[e][t] + gamma * k[e][t-1] * G[e][t-1],  k = 0 where done != 0 and 1 elsewhere; in front of t = 0 stands
          gamma * carry[e], and carry[e] leaves as k[e][T-1] * G[e][T-1]: a rollout continues the episodes the previous one left open
  batch   stats3 = {sum G, sum G^2, N T}, all-reduced over the ranks (a sum: the ranks then hold the same three numbers)
  merge   Chan's update of the running {mean, M2, count, skipped} by the batch; a batch with a non-finite sum is skipped and counted
  scale   1 / sqrt(M2 / count + eps), or 1 while there is no sample or no variance
  output  rew_n = clamp(rew * scale, -clip, clip) in f32

The statistics used for a rollout include that rollout (merge first, then scale).  The mean is tracked but not subtracted: a
shifted reward would change what an episode's length is worth.

return_traces / merge_running state the definitions sequentially in numpy: what the kernels (csrc/reward_norm.hip) are tested
against, and what a log reader replays a run with.
"""
from __future__ import annotations

import numpy as np
import torch

from . import ops
from .dist_utils import allreduce_sum

STATE_N = ops.RETNORM_STATE_N          # mean, M2, count, skipped


def check_reward_norm(reward_clip, reward_norm_gamma, gamma):
    """VecPPOTrainer's reward_clip / reward_norm_gamma -> (clip as a float, 0.0 = no clamp; the trace's gamma).  reward_clip: a
    positive finite number or None; reward_norm_gamma: None (the GAE's gamma) or a number in [0, 1].  Anything else raises
    ValueError.  Pure host arithmetic: VecPPOTrainer calls it before it allocates anything."""
    num = (int, float, np.integer, np.floating)
    if reward_clip is None:
        clip = 0.0
    else:
        if isinstance(reward_clip, bool) or not isinstance(reward_clip, num):
            raise ValueError(f"reward_clip={reward_clip!r}: a positive finite number, or None")
        clip = float(reward_clip)
        if not (clip > 0.0 and clip < float("inf")):
            raise ValueError(f"reward_clip={reward_clip!r}: a positive finite number, or None")
    g = gamma if reward_norm_gamma is None else reward_norm_gamma
    if isinstance(g, bool) or not isinstance(g, num) or not 0.0 <= float(g) <= 1.0:
        raise ValueError(f"reward_norm_gamma={g!r}: a number in [0, 1], or None for the GAE's gamma")
    return clip, float(g)


def return_traces(rew, done, gamma, carry):
    """(G f64 [N][T], carry_out f64 [N]) of rew / done [N][T] continued from carry [N]: the definition, one step after the other."""
    rew, done = np.asarray(rew, dtype=np.float64), np.asarray(done)
    N, T = rew.shape
    gamma = np.float64(gamma)
    G = np.empty((N, T), dtype=np.float64)
    left = np.array(carry, dtype=np.float64).reshape(N).copy()         # k * G of the step to the left
    for t in range(T):
        G[:, t] = rew[:, t] + gamma * left
        left = np.where(done[:, t] != 0, 0.0, 1.0) * G[:, t]
    return G, left


def batch_stats(G):
    """stats3 of a batch of traces: {sum G, sum G^2, count}."""
    G = np.asarray(G, dtype=np.float64)
    return np.array([G.sum(), (G * G).sum(), float(G.size)], dtype=np.float64)


def merge_running(state, stats3, eps=1e-8):
    """(new state f64 [4], scale f32) after the batch sums stats3 are merged into state = {mean, M2, count, skipped}: the lines
    of return_norm_merge_kernel, in its order of operations."""
    mean, M2, count, skipped = (np.float64(v) for v in np.asarray(state, dtype=np.float64).reshape(STATE_N))
    s, q, nb = (np.float64(v) for v in np.asarray(stats3, dtype=np.float64).reshape(3))
    if np.isfinite(s) and np.isfinite(q) and nb > 0.0:
        mb = s / nb
        M2b = max(q - s * s / nb, np.float64(0.0))
        d = mb - mean
        tot = count + nb
        mean = mean + d * nb / tot
        M2 = M2 + (M2b + d * d * count * nb / tot)
        count = tot
    else:
        skipped = skipped + 1.0
    scale = np.float32(1.0)
    if count > 0.0:
        var = M2 / count
        if var > 0.0:
            scale = np.float32(1.0 / np.sqrt(var + np.float64(eps)))
    return np.array([mean, M2, count, skipped], dtype=np.float64), scale


STATE_FILE = "reward_norm_state.npz"


def save_state(normaliser, model_path):
    """The training scripts: the normaliser's state_dict() (plus gamma, clip, eps) as reward_norm_state.npz beside the saved
    model; returns the path.  The running state is the same on every rank, the carry is the writing rank's."""
    import os
    path = os.path.join(os.path.dirname(model_path) or ".", STATE_FILE)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez(path, gamma=normaliser.gamma, clip=normaliser.clip, eps=normaliser.eps, **normaliser.state_dict())
    return path


class RewardNormaliser:
    """The trainer's collaborator for normalise_rewards=True (like RangeGuard): owns the open episodes' carry, the batch sums,
    the running state, the scale and the scaled copy rew_n -- the reward array it is given is never written."""

    def __init__(self, num_envs, horizon, gamma, clip, eps=1e-8, device="cuda"):
        self.N, self.T = int(num_envs), int(horizon)
        self.clip, self.gamma = check_reward_norm(clip, gamma, gamma)       # clip None: no clamp (0.0 to the kernel)
        self.eps = float(eps)
        if not self.eps > 0.0:
            raise ValueError(f"eps={eps!r}: a positive number")
        self.device = torch.device(device)
        f64 = dict(dtype=torch.float64, device=self.device)
        self.carry = torch.zeros(self.N, **f64)
        self.stats3 = torch.zeros(3, **f64)
        self.state = torch.zeros(STATE_N, **f64)
        self.scale = torch.ones(1, dtype=torch.float32, device=self.device)
        self.rew_n = torch.zeros(self.N, self.T, dtype=torch.float32, device=self.device)

    def __call__(self, rew, done):
        """rew, done f32 [N][T] of one rollout -> rew_n.  Four launches and one small all-reduce, nothing read by the host."""
        ops.return_stats(rew, done, self.carry, self.gamma, stats3=self.stats3)
        allreduce_sum(self.stats3)            # every rank merges the same whole-batch sums: the running state stays replicated
        ops.return_norm_merge(self.state, self.stats3, self.eps, scale=self.scale)
        return ops.reward_scale(rew, self.scale, self.clip, out=self.rew_n)

    def reset(self):
        self.carry.zero_()
        self.stats3.zero_()
        self.state.zero_()
        self.scale.fill_(1.0)

    def state_dict(self):
        return {"state": self.state.cpu().numpy(), "carry": self.carry.cpu().numpy()}

    def load_state_dict(self, sd):
        state, carry = np.asarray(sd["state"], dtype=np.float64).reshape(-1), np.asarray(sd["carry"], dtype=np.float64).reshape(-1)
        if state.size != STATE_N or carry.size != self.N:
            raise ValueError(f"reward normaliser state: {state.size} state values and a carry of {carry.size} envs for {self.N} envs")
        self.state.copy_(torch.from_numpy(state))
        self.carry.copy_(torch.from_numpy(carry))
        # the scale follows from the state (a merge of nothing would count a skip): restated on the host, as merge_running does
        mean, M2, count, _ = state
        var = M2 / count if count > 0.0 else 0.0
        self.scale.fill_(float(np.float32(1.0 / np.sqrt(var + self.eps))) if var > 0.0 else 1.0)

    def host_scale(self):
        """The scale in force (one host read)."""
        return float(self.scale.item())
