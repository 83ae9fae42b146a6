"""greedy.py -- what evaluate_with_lstm.py, evaluate_model.py and generate_expert_data.py share: which kind of policy an object is,
whether the fused greedy kernels cover it (fused_refusal), the policy_probs of the step-wise loop, and the fused chunk driver."""
from __future__ import annotations

import contextlib

import torch

from . import ops

F32 = torch.float32
_MLP_SHAPE = (256, 128, 5)               # h1, h2, n_act of the fused MLP kernels; their input width is 6 + trend_k


def policy_core(policy):
    """(kind, policy) of a policy object: "lstm" for LSTMActorCritic, "mlp" for MLPActorCritic or model.PPOActorCritic (an
    nn.Module, hence callable: the policy classes are recognised before anything is taken for a policy_probs function)."""
    from .policy import LSTMActorCritic, MLPActorCritic
    core = getattr(policy, "core", policy)
    if isinstance(core, LSTMActorCritic):
        return "lstm", core
    if isinstance(core, MLPActorCritic):
        return "mlp", core
    if callable(policy):
        return None
    raise TypeError(f"evaluate: expected a callable, LSTMActorCritic, MLPActorCritic or PPOActorCritic, got {type(policy).__name__}")


def _out_of_range(kind, core):
    """max |param| (NaN not counted) against the trainer's fp16-split limit: (value, limit, out of range)."""
    from .trainer import MLP_RANGE_LIMITS, RANGE_LIMITS
    limit = RANGE_LIMITS[0] if kind == "lstm" else MLP_RANGE_LIMITS[0]
    a = core.flat.detach().abs()
    pmax = float(torch.where(torch.isnan(a), torch.zeros_like(a), a).max())
    return pmax, limit, not pmax < limit


def fused_refusal(policy, env):
    """Why uav_greedy_episodes cannot run `policy` on `env` (None when it can)."""
    kind, core = policy_core(policy)
    mode = ops.get_lstm_arith(env.device)
    if mode != "fp16x3":
        return f"the handle's arithmetic is {mode}; the fused greedy kernels exist in fp16x3 only"
    trend = f" (the env has trend_k = {env.trend_k})" if env.trend_k else ""      # every refusal on a trend env names trend_k
    if kind == "lstm":
        if core.num_layers != 1 or core.hidden not in (64, 128) or core.n_act != 5:
            return (f"LSTM {core.num_layers} layer(s), hidden {core.hidden}, obs_dim {core.obs_dim}, {core.n_act} actions; "
                    f"the fused kernel covers one layer of hidden 64 / 128, obs_dim 6 + trend_k, 5 actions{trend}")
        if core.obs_dim != 6 + env.trend_k:
            return (f"the policy's obs_dim is {core.obs_dim}, the env's observations have {6 + env.trend_k} features "
                    f"(6 + trend_k, trend_k = {env.trend_k})")
    elif (core.h1, core.h2, core.n_act) != _MLP_SHAPE or not 6 <= core.in_dim <= 8:
        return (f"MLP {core.in_dim}-{core.h1}-{core.h2}-{core.n_act}; the fused kernel covers (6 + trend_k)-256-128-5 with "
                f"trend_k 0, 1 or 2 only{trend}")
    elif core.in_dim != 6 + env.trend_k:
        return (f"the MLP has {core.in_dim} inputs, the env's observations have {6 + env.trend_k} features "
                f"(6 + trend_k, trend_k = {env.trend_k})")
    # NaN parameters are not out of range: they reach the kernel and come back as nan_count ("NaN in probs")
    pmax, limit, out = _out_of_range(kind, core)
    if out:
        return f"max |param| = {pmax:g} is not below {limit:g}, the fp16-split range limit (uavppo/trainer.py)"
    return None


def stepwise_policy_probs(kind, core, env):
    """policy_probs for the step-wise loop: the LSTM's (h, c) start at zero and are carried through LSTMActorCritic.step.
    nan[0] counts steps whose logits hold a NaN among envs whose episode has not ended (env.done of the previous step).
    Parameters beyond the fp16-split range on a handle in that mode: the policy's own calls run in bf16x6, as the trainer
    switches (VecPPOTrainer._decide); the handle's mode is restored after each call, so the stop predictors keep theirs."""
    N, A = env.num_envs, core.n_act
    wide = ops.get_lstm_arith(env.device) == "fp16x3" and _out_of_range(kind, core)[2]
    nan = torch.zeros(1, dtype=torch.int64, device=env.device)
    live = torch.ones(N, dtype=torch.bool, device=env.device)
    state = core.zero_state(N) if kind == "lstm" else None
    work, calls = {}, [0]

    def probs(obs):
        if calls[0]:
            live.logical_and_(env.done <= 0.5)       # env.done of the previous step (stale before the first one)
        calls[0] += 1
        with ops.lstm_arith("bf16x6", env.device) if wide else contextlib.nullcontext():
            if kind == "lstm":
                logits = core.step(obs, state[0], state[1], work=work)[:, :A]
            else:
                logits = core.heads(obs.contiguous())[:, :A]
        nan.add_((torch.isnan(logits).any(1) & live).sum())
        return logits

    return probs, nan


class GreedyRun:
    """One greedy episode per environment of `env` (reset by the caller) on uav_greedy_episodes, or with `rule`
    (ops.make_stop_rule) on uav_greedy_episodes_stop, a chunk of steps per launch.  Owns what the launches carry along: the LSTM's
    h, c (None for the MLP), the kernel's `active` u8 [N] (cleared where an episode ends), nan_count, the rule's stop_win / stop_cnt."""

    def __init__(self, kind, core, env, rule=None):
        N, dev = env.num_envs, env.device
        self.core, self.env, self.rule = core, env, rule
        self.H = core.hidden if kind == "lstm" else 0
        self.trend = kind != "lstm" and env.trend_k != 0     # an MLP with 6 + trend_k inputs: policy_kind 2
        self.h = torch.zeros(N, self.H, dtype=F32, device=dev) if self.H else None
        self.c = torch.zeros(N, self.H, dtype=F32, device=dev) if self.H else None
        self.active = torch.ones(N, dtype=torch.uint8, device=dev)
        self.nan_count = torch.zeros(1, dtype=torch.int32, device=dev)
        self.stop_win = torch.zeros(N, rule.window, 2, dtype=F32, device=dev) if rule is not None else None
        self.stop_cnt = torch.zeros(N, dtype=torch.int32, device=dev) if rule is not None else None

    def chunk(self, t0, k, noise=None, rule_val=None):
        """Steps t0 + 1 .. t0 + k in one launch -> their records (ops.greedy_recs).  noise: optional f64 [steps, N, 2] of the
        whole run; rule_val: optional f32 [N, k] out (the rule's pos_std per step)."""
        env = self.env
        recs = ops.greedy_recs(env.num_envs, k, env.obs_dim, env.device)
        nz = None if noise is None else noise[t0:t0 + k].transpose(0, 1).contiguous()
        args = (env.state, env.num_envs, env.cfg(), self.core.flat, self.H, k, env.obs, self.h, self.c, self.active, recs)
        if self.rule is None:
            ops.greedy_episodes(*args, noise=nz, nan_count=self.nan_count, trend=self.trend)
        else:
            ops.greedy_episodes_stop(*args, self.rule, self.stop_win, self.stop_cnt, noise=nz, nan_count=self.nan_count,
                                     rule_val=rule_val, trend=self.trend)
        return recs

    def retire(self, active):
        """envs the host has ended (bool [N] of those still running) go into the next chunk inactive"""
        self.active &= active.to(torch.uint8)

    def raise_on_nan(self):
        if int(self.nan_count.item()) > 0:
            raise RuntimeError("NaN in probs")                                       # model.py:47-49
