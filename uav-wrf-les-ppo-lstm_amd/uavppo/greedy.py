"""greedy.py -- what evaluate_with_lstm.py, evaluate_model.py and generate_expert_data.py share: which kind of policy an object is,
whether the fused greedy kernels cover it (fused_refusal) or the per-step tail kernel does (tail_refusal), which of the three routes
a call takes (greedy_route), the policy_probs of the step-wise loop, and the chunk driver of the fused and the tail route."""
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
    from .range_guard import MLP_RANGE_LIMITS, RANGE_LIMITS
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


def tail_refusal(policy, env):
    """Why the tail route (the LSTM layers' step kernels + uav_greedy_tail per env step, GreedyRun(tail=True)) cannot run `policy`
    on `env` (None when it can): it covers every LSTMActorCritic of 5 actions whose hidden size is a multiple of 4 up to 256, in
    any arithmetic mode and parameter range."""
    kind, core = policy_core(policy)
    if kind != "lstm":
        return (f"MLP {core.in_dim}-{core.h1}-{core.h2}-{core.n_act}; the tail route (uav_greedy_tail) runs behind LSTM layers only")
    if core.n_act != 5 or core.hidden % 4 != 0 or not 4 <= core.hidden <= 256:
        return (f"LSTM {core.num_layers} layer(s), hidden {core.hidden}, {core.n_act} actions; uav_greedy_tail covers a hidden size "
                f"that is a multiple of 4 up to 256 and 5 actions")
    if core.obs_dim != 6 + env.trend_k:
        return (f"the policy's obs_dim is {core.obs_dim}, the env's observations have {6 + env.trend_k} features "
                f"(6 + trend_k, trend_k = {env.trend_k})")
    return None


def greedy_route(fused, tail, fused_why, tail_why, who="evaluate"):
    """"fused", "tail" or "stepwise" for the keywords fused / tail (None, True, False) of evaluate() and run_evaluation(), given
    what fused_refusal and tail_refusal said (None = covered).  fused=True: the fused kernels or a RuntimeError; else tail=True:
    the tail route or a RuntimeError; fused=None takes the fused kernels where they cover the policy; where they refuse it and
    tail is None too, the tail route where that covers it; everything else (fused=False alone among them) steps one launch
    sequence per time step."""
    if fused:
        if fused_why is not None:
            raise RuntimeError(f"{who}(fused=True): {fused_why}")
        return "fused"
    if tail:
        if tail_why is not None:
            raise RuntimeError(f"{who}(tail=True): {tail_why}")
        return "tail"
    if fused is None and fused_why is None:
        return "fused"
    if fused is None and tail is None and tail_why is None:
        return "tail"
    return "stepwise"


def policy_route(policy, env, fused=None, tail=None, who="evaluate"):
    """greedy_route for a policy object on `env`"""
    return greedy_route(fused, tail, fused_refusal(policy, env) if fused is not False else "fused=False",
                        tail_refusal(policy, env) if tail is not False else "tail=False", who)


def stepwise_policy_probs(kind, core, env):
    """policy_probs for the step-wise loop: the LSTM's (h, c) start at zero and are carried through LSTMActorCritic.step.
    nan[0] counts steps whose logits hold a NaN among envs whose episode has not ended (env.done of the previous step).
    Parameters beyond the fp16-split range on a handle in that mode: the policy's own calls run in bf16x6, as the trainer
    switches (RangeGuard._decide, uavppo/range_guard.py); the handle's mode is restored after each call, so the stop predictors keep theirs."""
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
    """One greedy episode per environment of `env` (reset by the caller), a chunk of steps per chunk() call and no host
    synchronisation inside it.  Two backends leave the same records:
      fused (default)  uav_greedy_episodes, or with `rule` (ops.make_stop_rule) uav_greedy_episodes_stop: a chunk is one launch;
      tail=True        per env step the LSTM layers (layers_step), then ONE uav_greedy_tail on the top layer's y (heads, argmax,
                       env step, the rule, the record).  h = 256 in the fp16-split arithmetic with parameters in range steps its
                       layers on ops.LstmStepper objects of this run (not the policy's, which belong to a trainer's rollout),
                       the upper layers reading the piece planes of the layer below.  A stepper carries its state from step t to
                       t + 1 of ONE [N, T] sequence (through the stash rows and its piece planes) and hands it out as hn / cn at
                       t = T - 1 only, so the run steps segments of SEG steps over [N, SEG] arrays, as a trainer's rollout does
                       over its horizon, and begins every further segment from the hn / cn of the one before; segments run on
                       across chunk() calls.  The observation goes into the segment's x row by one copy: L + 2 launches per step.
                       Everything else calls uav_lstm_fwd per layer as LSTMActorCritic.step does (in bf16x6 where the parameters
                       left the fp16-split range, the handle's mode restored after each step): 3 L + 1 launches.
    Owns what the launches carry along: the LSTM's h, c (None for the MLP; [L, N, H] on the tail route, where steppers keep theirs),
    the kernel's `active` u8 [N] (cleared where an episode ends), nan_count, the rule's stop_win / stop_cnt."""

    SEG = 16            # steps per stepper segment of the tail route: stash [N, SEG, 6H] per layer, one begin() per SEG steps

    def __init__(self, kind, core, env, rule=None, tail=False):
        N, dev = env.num_envs, env.device
        self.core, self.env, self.rule, self.tail = core, env, rule, bool(tail)
        self.H = core.hidden if kind == "lstm" else 0
        self.trend = kind != "lstm" and env.trend_k != 0     # an MLP with 6 + trend_k inputs: policy_kind 2
        self.h = torch.zeros(N, self.H, dtype=F32, device=dev) if self.H else None
        self.c = torch.zeros(N, self.H, dtype=F32, device=dev) if self.H else None
        self.active = torch.ones(N, dtype=torch.uint8, device=dev)
        self.nan_count = torch.zeros(1, dtype=torch.int32, device=dev)
        self.stop_win = torch.zeros(N, rule.window, 2, dtype=F32, device=dev) if rule is not None else None
        self.stop_cnt = torch.zeros(N, dtype=torch.int32, device=dev) if rule is not None else None
        if self.tail:
            self._begin_tail(kind)

    def _begin_tail(self, kind):
        core, env = self.core, self.env
        if kind != "lstm":
            raise RuntimeError("GreedyRun(tail=True): the tail route runs behind LSTM layers only")
        N, dev, H, L, v = env.num_envs, env.device, core.hidden, core.num_layers, core.views
        self.h, self.c = core.zero_state(N)
        self.wide = ops.get_lstm_arith(dev) == "fp16x3" and _out_of_range(kind, core)[2]
        self.steppers, self.work = None, {}
        if (H == 256 and not self.wide and ops.get_lstm_arith(dev) == "fp16x3"
                and ops.lstm_bwd_caps(dev, core.obs_dim, 256) != 0):      # 0: the handle is not on the fp16 step path
            self.steppers = [ops.LstmStepper(N, core.obs_dim if l == 0 else H, H, dev) for l in range(L)]
            S = self.SEG
            self.xseq = torch.zeros(N, S, core.obs_dim, dtype=F32, device=dev)
            self.y = [torch.empty(N, S, H, dtype=F32, device=dev) for _ in range(L)]
            self.stash = [torch.empty(N, S, 6 * H, dtype=F32, device=dev) for _ in range(L)]
            self.seg_t = 0                                   # the step of the current segment the next layers_step() runs
            self._begin_segment([(self.h[l], self.c[l]) for l in range(L)])

    def restart(self):
        """Start over for another run of episodes on the same env (reset by the caller) and the same policy object, whose
        parameters may have changed: h, c, active, nan_count, the rule's window and the tail's segment state as __init__ leaves
        them, in place -- nothing is reallocated and the host reads nothing."""
        if self.h is not None:
            self.h.zero_()
            self.c.zero_()
        self.active.fill_(1)
        self.nan_count.zero_()
        if self.stop_win is not None:
            self.stop_win.zero_()
            self.stop_cnt.zero_()
        if self.tail and self.steppers is not None:
            self.seg_t = 0
            self._begin_segment([(self.h[l], self.c[l]) for l in range(self.core.num_layers)])

    def _begin_segment(self, states):
        v = self.core.views
        for l, (sp, (h, c)) in enumerate(zip(self.steppers, states)):
            sp.begin(v[f"lstm.weight_ih_l{l}"], v[f"lstm.weight_hh_l{l}"], v[f"lstm.bias_ih_l{l}"], v[f"lstm.bias_hh_l{l}"], h, c)

    def layers_step(self):
        """The recurrent layers of one env step on env.obs, state carried from the step before -> the top layer's output, [N, H]
        rows (strided on the stepper backend) or [N, 1, H]: what LSTMActorCritic.step(want_heads=False) returns, bit for bit."""
        env = self.env
        if self.steppers is None:
            with ops.lstm_arith("bf16x6", env.device) if self.wide else contextlib.nullcontext():
                return self.core.step(env.obs, self.h, self.c, work=self.work, want_heads=False)
        j = self.seg_t
        self.xseq[:, j].copy_(env.obs)
        x = self.xseq
        for l, sp in enumerate(self.steppers):
            sp.step(x, j, self.y[l], self.stash[l], below=self.steppers[l - 1] if l > 0 else None)
            x = self.y[l]
        self.seg_t = (j + 1) % self.SEG
        if self.seg_t == 0:                                  # step SEG - 1 wrote hn / cn: the next segment starts from them
            self._begin_segment([(sp.hn, sp.cn) for sp in self.steppers])
        return x[:, j]

    def chunk(self, t0, k, noise=None, rule_val=None):
        """Steps t0 + 1 .. t0 + k (one launch on the fused backend) -> their records (ops.greedy_recs).  noise: optional f64
        [steps, N, 2] of the whole run; rule_val: optional f32 [N, k] out (the rule's pos_std per step)."""
        env = self.env
        recs = ops.greedy_recs(env.num_envs, k, env.obs_dim, env.device)
        if self.tail:
            return self._chunk_tail(t0, k, noise, rule_val, recs)
        nz = None if noise is None else noise[t0:t0 + k].transpose(0, 1).contiguous()
        args = (env.state, env.num_envs, env.cfg(), self.core.flat, self.H, k, env.obs, self.h, self.c, self.active, recs)
        if self.rule is None:
            ops.greedy_episodes(*args, noise=nz, nan_count=self.nan_count, trend=self.trend)
        else:
            ops.greedy_episodes_stop(*args, self.rule, self.stop_win, self.stop_cnt, noise=nz, nan_count=self.nan_count,
                                     rule_val=rule_val, trend=self.trend)
        return recs

    def _chunk_tail(self, t0, k, noise, rule_val, recs):
        core, env = self.core, self.env
        N, v, cfg = env.num_envs, core.views, env.cfg()
        for i in range(k):
            x = self.layers_step()
            ops.greedy_tail(env.state, cfg, x, v["head.weight"], v["head.bias"], i, env.obs, self.active, recs, self.nan_count,
                            noise=None if noise is None else noise[t0 + i], rule=self.rule, stop_win=self.stop_win,
                            stop_cnt=self.stop_cnt, rule_val=rule_val if self.rule is not None else None)
        return recs

    def retire(self, active):
        """envs the host has ended (bool [N] of those still running) go into the next chunk inactive"""
        self.active &= active.to(torch.uint8)

    def raise_on_nan(self):
        if int(self.nan_count.item()) > 0:
            raise RuntimeError("NaN in probs")                                       # model.py:47-49
