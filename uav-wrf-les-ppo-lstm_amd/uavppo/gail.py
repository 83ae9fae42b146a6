"""GAIL on the vectorised trainer: the reference's Discriminator (PPOV2.0/model.py:58-70) on the fused kernels of
csrc/disc.hip, and GAILTrainer, the loop of PPOV1.1/train_ppo_gail.py around VecPPOTrainer.

What the reference's script does per episode -- a PPO update, then ONE discriminator step on (whole expert set, the
episode's own states / actions), train_ppo_gail.py:150-175 -- GAILTrainer does per rollout.  One thing is added: the
reference trains its discriminator and then uses it nowhere, so its policy never sees an imitation signal; here the
rollout's reward is shaped as env_coef * r + gail_coef * softplus(z) = env_coef * r - gail_coef * log(1 - D) before GAE
(uav_disc_reward).  gail_coef = 0, env_coef = 1 is VecPPOTrainer bit for bit.

The policy side of the reference's GAIL script (train_ppo_gail.py:71-148: bootstrap at BATCH_SIZE boundaries, returns from
the raw advantage, shuffled row minibatches) is VecPPOTrainer's update_form="inline_v10" + minibatch_rows=B, which GAILTrainer
inherits (MLP policy); the default stays the project's _update_model path.

Out of scope: the TensorBoard histograms; PPOV1.1/evaluate_model.py; a multi-rank GPU test (the all-reduce is issued, and exercised under the
one-rank forced-collectives switch only).
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import ops
from .dist_utils import allreduce_grad, allreduce_sum
from .policy import _FlatPolicy
from .trainer import VecPPOTrainer

DISC_LR = 3e-5          # LEARNING_RATE of PPOV1.1/config.py:16, what train_ppo_gail.py:38 gives optimizer_d


def as_action_index(action, n_act):
    """Action indices i32 [n] from indices [n] (any integer dtype) or one-hot rows [n, n_act]; an all-zero row becomes -1
    (no one-hot column, as the kernels treat an out-of-range action)."""
    if action.dim() == 2:
        if action.shape[1] != n_act:
            raise RuntimeError(f"one-hot actions: expected [n, {n_act}], got {tuple(action.shape)}")
        idx = action.argmax(1)
        hot = torch.zeros_like(action).scatter_(1, idx[:, None], 1)
        zero = action.abs().sum(1) == 0
        if not bool(((action == hot) | zero[:, None]).all()):
            raise RuntimeError("actions must be indices or one-hot rows: the discriminator kernels build the one-hot columns themselves")
        return torch.where(zero, torch.full_like(idx, -1), idx).to(torch.int32)
    return action.reshape(-1).to(torch.int32)


class Discriminator(_FlatPolicy):
    """PPOV2.0/model.py:58-70: Linear(state_dim + action_dim, 128), ReLU, Linear(128, 1), Sigmoid over [state | one_hot(action)],
    as one flat f32 buffer in state_dict order (`.flat`, gradient in `.grad`); state_dict() / load_state_dict() use the
    reference's keys net.{0,2}.{weight,bias}, so it loads from and into the torch module.  Initialisation is nn.Linear's
    default (uniform in +-1/sqrt(fan_in) for weights and biases) drawn from a CPU generator seeded with `seed`."""
    HIDDEN = ops.DISC_HIDDEN
    KEYS = ("net.0.weight", "net.0.bias", "net.2.weight", "net.2.bias")

    def __init__(self, state_dim, action_dim, device="cuda", seed=None):
        self.state_dim, self.action_dim = int(state_dim), int(action_dim)
        H, I = self.HIDDEN, self.state_dim + self.action_dim
        n = ops.disc_param_count(self.state_dim, self.action_dim, H)          # refuses shapes the kernels do not take
        self._alloc([("net.0.weight", (H, I)), ("net.0.bias", (H,)), ("net.2.weight", (1, H)), ("net.2.bias", (1,))], device)
        assert self.flat.numel() == n
        gen = torch.Generator().manual_seed(seed) if seed is not None else None
        for name, shape in self.layout:
            bound = 1.0 / math.sqrt(I if name.startswith("net.0") else H)
            self.views[name].copy_(torch.empty(shape).uniform_(-bound, bound, generator=gen))

    def state_dict(self):
        return {k: self.views[k].detach().clone() for k in self.KEYS}

    def load_state_dict(self, sd):
        for k in self.KEYS:
            self.views[k].copy_(torch.as_tensor(sd[k], dtype=torch.float32).reshape(self.views[k].shape))

    def parameters(self):
        return [self.views[k] for k in self.KEYS]

    def _rows(self, state, action):
        s = torch.as_tensor(state).to(self.device, torch.float32).reshape(-1, self.state_dim).contiguous()
        a = as_action_index(torch.as_tensor(action).to(self.device), self.action_dim).contiguous()
        if a.numel() != s.shape[0]:
            raise RuntimeError(f"discriminator: {s.shape[0]} states, {a.numel()} actions")
        return s, a

    def neg_log_one_minus_d(self, state, action):
        """softplus(z) = -log(1 - D) [n], from the logit (uav_disc_reward with env_coef 0, gail_coef 1)."""
        s, a = self._rows(state, action)
        return ops.disc_reward(self.flat, s, a, self.action_dim)

    def __call__(self, state, action):
        """D [n, 1] on the caller's device; action: one-hot rows [n, action_dim] (the reference's call) or indices [n].
        D = 1 - exp(-softplus(z)), taken as -expm1 so that a small D keeps its digits."""
        src = torch.as_tensor(state).device
        return (-torch.expm1(-self.neg_log_one_minus_d(state, action))).reshape(-1, 1).to(src)

    forward = __call__


def load_expert(expert, device):
    """(states f32 [M, obs_dim], actions i32 [M]) on `device` from a pair of arrays / tensors or the path of an .npz with the
    reference's keys `states`, `actions` (generate_expert_data.py:58)."""
    if isinstance(expert, (str, bytes)) or hasattr(expert, "__fspath__"):
        data = np.load(expert)
        expert = (data["states"], data["actions"])
    s = torch.as_tensor(np.asarray(expert[0]) if not torch.is_tensor(expert[0]) else expert[0])
    a = torch.as_tensor(np.asarray(expert[1]) if not torch.is_tensor(expert[1]) else expert[1])
    s = s.to(device, torch.float32).contiguous()
    a = a.to(device).reshape(-1).to(torch.int32).contiguous()
    if s.dim() != 2 or s.shape[0] != a.numel() or s.shape[0] == 0:
        raise RuntimeError(f"expert data: states {tuple(s.shape)}, actions {tuple(a.shape)}")
    return s, a


class GAILTrainer(VecPPOTrainer):
    """VecPPOTrainer + a discriminator.  train_iteration(): collect(); the shaped reward env_coef * rew + gail_coef * softplus(z)
    of this rollout's (obs, act) into `rew_shaped` (buf["rew"] stays the environment's: CSV and trajectory logs unchanged); GAE on
    it; the unchanged PPO update; then disc_steps x (uav_disc_grad on (whole expert set, this rollout's obs / act), gradient
    all-reduce with global counts, uav_clip_adam with clipping off on the discriminator's own moments); curriculum.  Policy first,
    discriminator afterwards, as train_ppo_gail.py:71-175.  The expert set is replicated on every rank."""

    def __init__(self, num_envs, horizon, policy="lstm", expert=None, gail_coef=1.0, env_coef=1.0, disc_lr=DISC_LR, disc_steps=1,
                 discriminator=None, **kw):
        super().__init__(num_envs, horizon, policy, **kw)
        if expert is None:
            raise ValueError("GAILTrainer: expert=(states, actions) or the path of an expert_data.npz is required")
        self.expert_obs, self.expert_act = load_expert(expert, self.device)
        if self.expert_obs.shape[1] != self.obs_dim:
            raise RuntimeError(f"expert states have {self.expert_obs.shape[1]} features, the policy observes {self.obs_dim}")
        self.n_act = 5
        self.disc = discriminator or Discriminator(self.obs_dim, self.n_act, self.device, seed=self.seed + 1)
        self.gail_coef, self.env_coef = float(gail_coef), float(env_coef)
        self.disc_lr, self.disc_steps = float(disc_lr), int(disc_steps)
        self.rew_shaped = torch.zeros_like(self.buf["rew"])
        self.disc_exp_avg = torch.zeros_like(self.disc.flat)
        self.disc_exp_avg_sq = torch.zeros_like(self.disc.flat)
        self.disc_opt_step = 0
        self.disc_sums = torch.zeros(4, dtype=torch.float64, device=self.device)
        self.disc_log = []           # with record: (loss_sums, gradient, parameters it was taken at) of every discriminator step

    def _rows(self):
        return self.buf["obs"].view(self.N * self.T, self.obs_dim), self.buf["act"].view(-1)

    def shape_reward(self):
        obs, act = self._rows()
        ops.disc_reward(self.disc.flat, obs, act, self.n_act, self.gail_coef, self.env_coef, rew_env=self.buf["rew"].view(-1),
                        out=self.rew_shaped.view(-1))
        return self.rew_shaped

    def _gae_reward(self):                  # compute_advantages(): the GAE reads the shaped reward
        return self.shape_reward()

    def update_discriminator(self):
        obs, act = self._rows()
        M = self.expert_obs.shape[0]
        for _ in range(self.disc_steps):
            ops.disc_grad(self.disc.flat, self.expert_obs, self.expert_act, obs, act, self.n_act, inv_ne=1.0 / (M * self.world),
                          inv_np=1.0 / (self.N * self.T * self.world), loss_sums=self.disc_sums, grad=self.disc.grad)
            allreduce_grad(self.disc.grad)
            if self.record:
                self.disc_log.append((self.disc_sums.clone(), self.disc.grad.clone(), self.disc.flat.clone()))
            self.disc_opt_step += 1
            ops.clip_adam(self.disc.flat, self.disc.grad, self.disc_exp_avg, self.disc_exp_avg_sq, self.disc_opt_step, self.disc_lr,
                          max_norm=0.0)
        return self.disc_sums

    def _after_update(self):                # train_iteration(): policy first, discriminator afterwards, then the curriculum
        self.update_discriminator()

    def disc_losses(self):
        """(expert loss, policy loss, accuracy) of the LAST discriminator step; raises on a NaN logit (or an action outside the
        action set), on every rank together, like losses()."""
        t = self.disc_sums.clone()
        if self._coll:
            allreduce_sum(t)
        s = t.cpu().numpy()
        if s[3] > 0:
            raise RuntimeError("NaN in discriminator output")
        M, n = self.expert_obs.shape[0] * self.world, self.N * self.T * self.world
        return s[0] / M, s[1] / n, s[2] / (M + n)
