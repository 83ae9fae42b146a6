"""ObsNormaliser: running per-channel observation normalisation (the observation half of "VecNormalize"), folded into the
policy's first affine layer, with no host read on the path.

The environment emits conc = o[2] in [0, 100] and its trend differences o[6], o[7] beside channels scaled to O(1).  Per channel
x^ = (x - mu) / sigma is affine and the first thing every policy here does with an observation is an affine map (w, b), so

  fold         w_eff[:, j] = w[:, j] * inv_sigma_j      b_eff = b - sum_j w_eff[:, j] mu_j        w_eff x + b_eff = w x^ + b
  unfold_grad  dw[:, j] = (dw_eff[:, j] - db_eff mu_j) * inv_sigma_j      db = db_eff             (the chain rule back)

and every kernel that reads an observation -- rollout, greedy, tail, forward, BPTT, MLP -- runs unchanged on RAW observations
with (w_eff, b_eff).  policy.flat always holds the folded, deployable parameters: rollouts, evaluation, state_dict() and the
saved model need nothing else.  The normaliser owns `master`, the flat buffer Adam updates; the two differ in the first layer's
weight and bias only (lstm.weight_ih_l0 / lstm.bias_ih_l0, or feature.0.weight / feature.0.bias).

Definitions (f64), obs f32 [rows][D] of one rollout:
  batch   stats = {rows, sum_j x, sum_j x^2}, in ONE order of summation for every shape (batch_stats), all-reduced over the ranks
  merge   Chan's update per channel of the running {count, skipped, mean_j, M2_j}; a batch with a non-finite sum is skipped whole
          and counted (merge_running)
  output  mu_j = f32(mean_j), inv_sigma_j = f32(1 / sqrt(M2_j / count + eps)); mu = 0, inv_sigma = 1 while count == 0 and for a
          channel that is masked out

Order of events (VecNormalize's): rollout k and ALL epochs of update k run on the same statistics S_k, so the PPO ratio is 1 at
the first step and the forward pass adopted from the fused rollout stays valid.  Behind the last optimiser step of update k the
rollout's observations are merged (S_k -> S_k+1) and the master is folded again.  S_0 is the identity.  Unlike the reward scale
(reward_norm.py: merge first, then scale), the statistics in force for a rollout can NOT include that rollout: its actions were
drawn before its observations could be counted.

eps defaults to 1e-4, not VecNormalize's 1e-8: the folded form has no place to clamp x^ (VecNormalize clips to +-10; a clamp is
not affine), so inv_sigma <= 1 / sqrt(eps) = 100 is all that bounds a channel that is constant so far -- o[5], the curriculum
radius, with the curriculum off -- on the day it moves.  When the statistics move, the function the master parameters stand for
moves with them (as under VecNormalize); nothing re-parametrises the master to keep it.

batch_stats / merge_running / fold / unfold_grad / unfold state the kernels (csrc/obs_norm.hip) in numpy: what they are tested
against, and what a log reader replays a run with.
"""
from __future__ import annotations

import numpy as np
import torch

from . import ops
from .dist_utils import allreduce_sum

SLOTS = 65536             # csrc/obs_norm.hip: 256 blocks of 256 threads, whatever the shape
STATE_FILE = "obs_norm_state.npz"
FIRST_LAYER = {"lstm": ("lstm.weight_ih_l0", "lstm.bias_ih_l0"), "mlp": ("feature.0.weight", "feature.0.bias")}


def check_obs_norm(normalise_obs, obs_norm_eps, obs_norm_channels, obs_dim):
    """VecPPOTrainer's normalise_obs / obs_norm_eps / obs_norm_channels -> (on, eps, mask): a bool; a positive finite float; the
    bit mask of the channels that are normalised (None: all obs_dim of them).  Anything else raises ValueError.  Pure host
    arithmetic: VecPPOTrainer calls it before it allocates anything."""
    if not isinstance(normalise_obs, (bool, np.bool_)):
        raise ValueError(f"normalise_obs={normalise_obs!r}: True or False")
    if isinstance(obs_norm_eps, bool) or not isinstance(obs_norm_eps, (int, float, np.integer, np.floating)):
        raise ValueError(f"obs_norm_eps={obs_norm_eps!r}: a positive finite number")
    eps = float(obs_norm_eps)
    if not (eps > 0.0 and eps < float("inf")):
        raise ValueError(f"obs_norm_eps={obs_norm_eps!r}: a positive finite number")
    D = int(obs_dim)
    if normalise_obs and not 6 <= D <= 8:
        raise ValueError(f"normalise_obs with {D} observation channels: the fold kernels take 6 .. 8 (trend_k 0 .. 2)")
    if obs_norm_channels is None:
        return bool(normalise_obs), eps, (1 << D) - 1
    if isinstance(obs_norm_channels, (str, bytes)):
        raise ValueError(f"obs_norm_channels={obs_norm_channels!r}: an iterable of channel indices, or None")
    try:
        chans = list(obs_norm_channels)
    except TypeError:
        raise ValueError(f"obs_norm_channels={obs_norm_channels!r}: an iterable of channel indices, or None") from None
    mask = 0
    for c in chans:
        if isinstance(c, bool) or not isinstance(c, (int, np.integer)) or not 0 <= int(c) < D:
            raise ValueError(f"obs_norm_channels: {c!r} is no channel index in [0, {D})")
        mask |= 1 << int(c)
    return bool(normalise_obs), eps, mask


def _tree(v):
    """wave_sum's tree over axis -2 (64 lanes -> lane 0), the kernel's shuffle-down order."""
    v = v.copy()
    o = 32
    while o > 0:
        v[..., :o, :] = v[..., :o, :] + v[..., o:2 * o, :]
        o >>= 1
    return v[..., 0, :]


def _block256(v):
    """block256_sum over axis -2 of [..., 256, C]: the tree per wave of 64, then ((w0 + w1) + w2) + w3."""
    w = _tree(v.reshape(v.shape[:-2] + (4, 64, v.shape[-1])))
    return ((w[..., 0, :] + w[..., 1, :]) + w[..., 2, :]) + w[..., 3, :]


def batch_stats(obs):
    """stats f64 [1 + 2 D] = {rows, channel sums, channel sums of squares} of obs [rows][D], summed as uav_obs_stats sums: slot
    k of 65536 takes the rows k, k + 65536, ... one after the other; the 256 slots of a block are added by block256_sum's tree,
    and so are the 256 block sums."""
    x = np.asarray(obs, dtype=np.float64)
    x = x.reshape(-1, x.shape[-1])
    rows, D = x.shape
    acc = np.zeros((SLOTS, 2 * D), dtype=np.float64)
    for r0 in range(0, rows, SLOTS):
        c = x[r0:r0 + SLOTS]
        acc[:c.shape[0], :D] += c
        acc[:c.shape[0], D:] += c * c
    total = _block256(_block256(acc.reshape(256, 256, 2 * D)))
    return np.concatenate([[np.float64(rows)], total])


def merge_running(state, stats, eps=1e-4, mask=None):
    """(new state f64 [2 + 2 D], mu f32 [D], inv_sigma f32 [D]) after the batch sums `stats` are merged into state = {count,
    skipped, mean_j, M2_j}: the lines of obs_norm_merge_kernel, in its order of operations.  mask: bit j set = channel j is
    normalised (None: every channel)."""
    stats = np.asarray(stats, dtype=np.float64).reshape(-1)
    D = (stats.size - 1) // 2
    st = np.array(state, dtype=np.float64).reshape(2 + 2 * D).copy()
    mask = (1 << D) - 1 if mask is None else int(mask)
    count, nb = st[0], stats[0]
    if nb > 0.0 and np.isfinite(stats[1:]).all():
        tot = count + nb
        for j in range(D):
            s, q = stats[1 + j], stats[1 + D + j]
            mean, M2 = st[2 + j], st[2 + D + j]
            mb = s / nb
            M2b = max(q - s * s / nb, np.float64(0.0))
            d = mb - mean
            st[2 + j] = mean + d * nb / tot
            st[2 + D + j] = M2 + (M2b + d * d * count * nb / tot)
        count = tot
        st[0] = count
    else:
        st[1] += 1.0
    mu, inv_sigma = np.zeros(D, dtype=np.float32), np.ones(D, dtype=np.float32)
    for j in range(D):
        if count > 0.0 and (mask >> j) & 1:
            mu[j] = np.float32(st[2 + j])
            inv_sigma[j] = np.float32(1.0 / np.sqrt(st[2 + D + j] / count + np.float64(eps)))
    return st, mu, inv_sigma


def fold(w, b, mu, inv_sigma):
    """(w_eff, b_eff) f32 of the master first layer w [rows][D], b [rows]: w_eff = f32(w * inv_sigma); b_eff = f32(b - sum_j
    w_eff_j mu_j), the sum in f64 with j ascending, one subtraction per channel."""
    w, b = np.asarray(w, dtype=np.float32), np.asarray(b, dtype=np.float32)
    mu, inv_sigma = np.asarray(mu, dtype=np.float32), np.asarray(inv_sigma, dtype=np.float32)
    w_eff = (w * inv_sigma[None, :]).astype(np.float32)
    acc = b.astype(np.float64)
    for j in range(w.shape[1]):
        acc = acc - w_eff[:, j].astype(np.float64) * np.float64(mu[j])
    return w_eff, acc.astype(np.float32)


def unfold_grad(dw, db, mu, inv_sigma):
    """dw f32 [rows][D] of the master weight from the folded one's gradient: f32((dw_j - db mu_j) * inv_sigma_j) in f64."""
    dw, db = np.asarray(dw, dtype=np.float32).astype(np.float64), np.asarray(db, dtype=np.float32).astype(np.float64)
    mu, inv_sigma = np.asarray(mu, dtype=np.float32).astype(np.float64), np.asarray(inv_sigma, dtype=np.float32).astype(np.float64)
    return ((dw - db[:, None] * mu[None, :]) * inv_sigma[None, :]).astype(np.float32)


def unfold(w_eff, b_eff, mu, inv_sigma):
    """(w, b) f32 with fold(w, b) = (w_eff, b_eff) up to rounding: w = f32(w_eff / inv_sigma), b = f32(b_eff + sum_j w_eff_j mu_j)."""
    w_eff, b_eff = np.asarray(w_eff, dtype=np.float32), np.asarray(b_eff, dtype=np.float32)
    mu, inv_sigma = np.asarray(mu, dtype=np.float32), np.asarray(inv_sigma, dtype=np.float32)
    acc = b_eff.astype(np.float64)
    for j in range(w_eff.shape[1]):
        acc = acc + w_eff[:, j].astype(np.float64) * np.float64(mu[j])
    return (w_eff / inv_sigma[None, :]).astype(np.float32), acc.astype(np.float32)


def save_state(normaliser, model_path):
    """The training scripts: the normaliser's state_dict() (plus eps and the channel mask) as obs_norm_state.npz beside the
    saved model; returns the path.  The saved model itself holds the folded parameters and needs this file for nothing but
    a continued training run."""
    import os
    path = os.path.join(os.path.dirname(model_path) or ".", STATE_FILE)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez(path, eps=normaliser.eps, mask=normaliser.mask, **normaliser.state_dict())
    return path


class ObsNormaliser:
    """The trainer's collaborator for normalise_obs=True (like RewardNormaliser and RangeGuard): owns the running state, mu /
    inv_sigma and `master`, the flat parameters Adam updates; keeps policy.flat = fold(master).  The observation array it is
    given is only read."""

    def __init__(self, policy, kind, eps=1e-4, mask=None, device="cuda"):
        self.policy, self.device = policy, torch.device(device)
        self.eps = float(eps)
        if not self.eps > 0.0:
            raise ValueError(f"eps={eps!r}: a positive number")
        wname, bname = FIRST_LAYER[kind]
        self.rows, self.D = (int(v) for v in policy.views[wname].shape)
        self.mask = (1 << self.D) - 1 if mask is None else int(mask)
        o, off = 0, {}
        for name, shape in policy.layout:
            off[name] = o
            o += int(np.prod(shape))
        self._ow, self._ob = off[wname], off[bname]
        # policy.flat through a tensor with a version counter of its own: the normaliser's writes are not "someone else wrote
        # the parameters" to the range guard or to itself (flat._version is how both see load_state_dict)
        self._flat = policy.flat.data
        self.master = torch.zeros_like(policy.flat)
        self.w_eff, self.b_eff = self._slices(self._flat)
        self.w, self.b = self._slices(self.master)
        self.stats = torch.zeros(1 + 2 * self.D, dtype=torch.float64, device=self.device)
        self.state = torch.zeros(ops.obs_norm_state_n(self.D), dtype=torch.float64, device=self.device)
        self.mu = torch.zeros(self.D, dtype=torch.float32, device=self.device)
        self.inv_sigma = torch.ones(self.D, dtype=torch.float32, device=self.device)
        self.frozen = False
        self.flat_version = -1
        self.reset()

    def _slices(self, flat):
        n = self.rows * self.D
        return flat[self._ow:self._ow + n].view(self.rows, self.D), flat[self._ob:self._ob + self.rows]

    def reset(self):
        """The statistics back to the identity; the policy keeps computing what it computes: master <- policy.flat."""
        self.stats.zero_()
        self.state.zero_()
        self.mu.zero_()
        self.inv_sigma.fill_(1.0)
        self.master.copy_(self._flat)
        self.flat_version = self.policy.flat._version

    def freeze(self):
        """Stop merging rollouts into the statistics (the fold of every optimiser step goes on: Adam keeps moving the master)."""
        self.frozen = True

    def unfreeze(self):
        self.frozen = False

    def sync_master(self):
        """Someone else wrote policy.flat (load_state_dict, an initial model: torch bumped flat._version): those are folded
        parameters, and the master that folds to them under the statistics in force is their unfold.  Returns whether it did."""
        if self.policy.flat._version == self.flat_version:
            return False
        self.master.copy_(self._flat)
        ops.obs_unfold(self.w_eff, self.b_eff, self.mu, self.inv_sigma, self.w, self.b)
        self.flat_version = self.policy.flat._version
        return True

    def unfold_grad(self, grad):
        """Optimiser step, behind the gradient all-reduce: the flat gradient (taken at policy.flat) becomes the master's."""
        self.sync_master()
        n = self.rows * self.D
        ops.obs_unfold_grad(grad[self._ow:self._ow + n].view(self.rows, self.D), grad[self._ob:self._ob + self.rows], self.mu,
                            self.inv_sigma)

    def fold(self, pmax=None):
        """policy.flat <- fold(master): the parameters beyond the first layer copied, the first layer folded; pmax (the range
        guard's slot, which uav_clip_adam just wrote from the master) raised to what the kernels will read."""
        self._flat.copy_(self.master)
        ops.obs_fold(self.w, self.b, self.mu, self.inv_sigma, self.w_eff, self.b_eff, pmax)

    def after_update(self, obs, pmax=None):
        """Behind the last optimiser step of an update: this rollout's observations into the statistics, then the fold under
        the new ones.  Statistics (a 4-byte memset and one launch), one small all-reduce, the merge, the flat copy and the
        fold; nothing is read by the host.  Frozen, the statistics stay and the last optimiser step's fold stands: nothing is
        launched, unless a foreign write had to be taken in."""
        synced = self.sync_master()
        if not self.frozen:
            ops.obs_stats(obs, self.stats)
            allreduce_sum(self.stats)             # every rank merges the same whole-batch sums: the running state stays replicated
            ops.obs_norm_merge(self.state, self.stats, self.mask, self.eps, self.mu, self.inv_sigma)
        if synced or not self.frozen:
            self.fold(pmax)

    def state_dict(self):
        self.sync_master()
        # mu / inv_sigma travel as the device wrote them: restated from `state` on the host, sqrt and the division could differ
        # in the last place, and policy.flat after a reload would not be the model that was saved
        return {"state": self.state.cpu().numpy(), "master": self.master.cpu().numpy(), "mu": self.mu.cpu().numpy(),
                "inv_sigma": self.inv_sigma.cpu().numpy(), "frozen": np.array(self.frozen)}

    def load_state_dict(self, sd):
        """The running state, mu / inv_sigma and the master, bit for bit; policy.flat becomes their fold: the saved model."""
        state, master = np.asarray(sd["state"], dtype=np.float64).reshape(-1), np.asarray(sd["master"], dtype=np.float32).reshape(-1)
        mu, inv = (np.asarray(sd[k], dtype=np.float32).reshape(-1) for k in ("mu", "inv_sigma"))
        if state.size != self.state.numel() or master.size != self.master.numel() or mu.size != self.D or inv.size != self.D:
            raise ValueError(f"observation normaliser state: {state.size} state values, {mu.size} / {inv.size} channel values and "
                             f"{master.size} parameters for {self.D} channels and {self.master.numel()} parameters")
        self.state.copy_(torch.from_numpy(state))
        self.master.copy_(torch.from_numpy(master))
        self.mu.copy_(torch.from_numpy(mu))
        self.inv_sigma.copy_(torch.from_numpy(inv))
        if "frozen" in sd:
            self.frozen = bool(np.asarray(sd["frozen"]))
        self.policy.flat.copy_(self.master)      # through the policy's own tensor: the range guard measures loaded parameters anew
        ops.obs_fold(self.w, self.b, self.mu, self.inv_sigma, self.w_eff, self.b_eff)
        self.flat_version = self.policy.flat._version

    def host_stats(self):
        """The statistics in force (one host read): count, skipped, mean [D], var [D] (M2 / count), mu [D], inv_sigma [D]."""
        t = torch.cat([self.state, self.mu.double(), self.inv_sigma.double()]).cpu().numpy()
        D, count = self.D, t[0]
        return {"count": float(count), "skipped": float(t[1]), "mean": t[2:2 + D].copy(),
                "var": t[2 + D:2 + 2 * D] / count if count > 0.0 else np.zeros(D),
                "mu": t[2 + 2 * D:2 + 3 * D].astype(np.float32), "inv_sigma": t[2 + 3 * D:].astype(np.float32)}
