"""VecPPOTrainer: the PPOV2.0/2.1 training loop (train_ppo2.0.py:110-261) for N vectorised
environments -- rollout collection, GAE, whole-buffer advantage normalisation, EPOCHS passes
of the clipped-PPO update -- every arithmetic step a HIP kernel behind the C ABI.

One process per GPU: environments are sharded by contiguous global index, parameters are
replicated, and per optimiser step ONE all-reduce (RCCL over xGMI) of the flat gradient buffer
keeps them identical; 3 doubles are all-reduced for the reference's whole-buffer advantage
statistics (train_ppo2.0.py:35-39).
"""
from __future__ import annotations

import os

import numpy as np
import torch

from . import ops
from .curriculum_link import CurriculumLink
from .dist_utils import allreduce_adv_stats, allreduce_grad, allreduce_sum, collectives_on, env_shard
from .policy import LSTMActorCritic, MLPActorCritic
from .eval_track import EvalTracker, check_eval
from .source_fit import option as source_fit_option
from .source_stop import option as source_stop_option
from .lr_control import LrController, check_lr_control, linear_value
from .range_guard import RangeGuard
from .obs_norm import ObsNormaliser, check_obs_norm
from .reward_norm import RewardNormaliser, check_reward_norm

# reference hyper-parameters, PPOV2.0/config.py:12-18 and train_ppo2.0.py:87,114
DEFAULTS = dict(gamma=0.99, lam=0.95, clip=0.2, ent_beta=0.01, lr=3e-5, epochs=5, max_grad_norm=0.5)


def chunk_plan(num_envs, horizon, num_minibatches, bptt_len, policy="lstm", minibatch_rows=None):
    """Truncated BPTT's cut of a rank's buffer: the [N][T] samples seen as N * C sequences of bptt_len consecutive steps
    (C = T / bptt_len chunk rows per env, row n * C + k = steps [k * bptt_len, (k + 1) * bptt_len) of env n), minibatch m the
    chunk rows [m R, (m + 1) R).  Returns (C, R); raises ValueError, with the reason, for what cannot be cut that way.  Pure
    host arithmetic: VecPPOTrainer calls it before it touches a device."""
    N, T, M, Lc = int(num_envs), int(horizon), int(num_minibatches), int(bptt_len)
    if minibatch_rows is not None:
        raise ValueError("bptt_len and minibatch_rows are two ways to cut the buffer (sequences of bptt_len steps / single sample "
                         "rows of the MLP): give one of them")
    if policy != "lstm":
        raise ValueError(f"bptt_len needs the LSTM policy: the {policy!r} policy carries no recurrent state through time to truncate")
    if Lc < 1:
        raise ValueError(f"bptt_len={bptt_len}: at least 1 step")
    if Lc > T:
        raise ValueError(f"bptt_len={Lc} is longer than the horizon of {T} steps")
    if T % Lc:
        raise ValueError(f"bptt_len={Lc} does not divide the horizon of {T} steps (chunks are whole)")
    C = T // Lc
    if (N * C) % M:
        raise ValueError(f"num_envs * horizon / bptt_len = {N * C} chunk rows are not divisible by num_minibatches={M} "
                         "(minibatches are whole chunk rows)")
    return C, N * C // M


def check_options(num_envs, horizon, policy, trend_k, update_form, gae_mode, num_minibatches, minibatch_rows, shuffle_envs, bptt_len):
    """VecPPOTrainer's keywords that cut or shuffle the buffer, refused where they contradict each other.  Returns
    (gae_mode, minibatch_rows, C): the GAE mode in force, the row count as an int or None, the chunk rows per env (chunk_plan;
    1 = full BPTT).  Pure host arithmetic, like chunk_plan: VecPPOTrainer calls it before it allocates anything."""
    N, M = int(num_envs), int(num_minibatches)
    # update_form "inline_v10": the inline update of PPOV1.1/train_ppo1.0.py:63-141 (also the policy side of
    # train_ppo_gail.py:71-148) instead of _update_model's arithmetic -- GAE with a real bootstrap V(next_state) on the last
    # step, returns from the raw advantage, (A - mean) / (std + 1e-8) without a guard.  It sets the GAE mode itself (a gae_mode other than the default beside it is refused).
    if update_form not in ("update_model", "inline_v10"):
        raise ValueError(f"update_form {update_form!r}: 'update_model' or 'inline_v10'")
    if update_form == "inline_v10" and gae_mode not in ("reference_exact", "inline_v10"):
        raise ValueError(f"update_form='inline_v10' runs its own GAE (uav_gae mode inline_v10); gae_mode={gae_mode!r} would be ignored")
    # minibatch_rows = B: every epoch one permutation of this rank's N * T sample rows, cut into chunks of B (the last one
    # shorter, as Tensor.split), each chunk one optimiser step (train_ppo1.0.py:92-136) through uav_mlp_ppo_grad_rows
    rows = None if minibatch_rows is None else int(minibatch_rows)
    if rows is not None:
        if M != 1:
            raise ValueError("num_minibatches and minibatch_rows are two ways to cut the buffer: give one of them")
        if rows < 1:
            raise ValueError(f"minibatch_rows={minibatch_rows}: a positive row count")
        if policy != "mlp" or not 6 <= 6 + int(trend_k) <= 8:
            raise ValueError("minibatch_rows needs the MLP policy on the fused path (6-256-128 with trend_k 0..2): only "
                             "uav_mlp_ppo_grad_rows reads its samples through a row index; an LSTM's samples are whole "
                             "env sequences (shuffle_envs=True shuffles those)")
    # shuffle_envs: every epoch one permutation of this rank's N envs, cut into num_minibatches chunks of N / M whole env
    # sequences; a chunk is packed into contiguous buffers by ONE launch (uav_gather_rows_multi) and the update's kernels run
    # on the packed minibatch unchanged
    if shuffle_envs:
        if rows is not None:
            raise ValueError("shuffle_envs and minibatch_rows are two ways to shuffle the buffer (whole env sequences / single "
                             "sample rows): give one of them")
        if M == 1:
            raise ValueError("shuffle_envs with num_minibatches=1: one minibatch of all envs leaves nothing to shuffle")
    # bptt_len = Lc (truncated BPTT, LSTM only): the update runs on the N * C sequences of Lc consecutive steps the buffer
    # holds (C = T / Lc), each started from the recurrent state the rollout's parameters give at its first step
    # (_chunk_start_states, once per iteration) -- gradients do not cross a chunk boundary.  The sample arrays are
    # contiguous, so the chunk view [N * C][Lc] is a reshape; the sequence kernels run on it unchanged.  None, or Lc = T
    # (one chunk per env), is full BPTT: the path without the keyword.
    C = 1 if bptt_len is None else chunk_plan(N, horizon, M, bptt_len, policy, rows)[0]
    if C == 1 and N % M:
        raise ValueError("num_envs must be divisible by num_minibatches (minibatches are whole env sequences)")
    if policy not in ("lstm", "mlp"):
        raise ValueError(policy)
    return "inline_v10" if update_form == "inline_v10" else gae_mode, rows, C


def check_target_kl(target_kl):
    """target_kl as a float, or None (no early stop); anything but a positive finite number is refused."""
    if target_kl is None:
        return None
    if isinstance(target_kl, bool) or not isinstance(target_kl, (int, float, np.integer, np.floating)):
        raise ValueError(f"target_kl={target_kl!r}: a positive finite number, or None")
    v = float(target_kl)
    if not (v > 0.0 and v < float("inf")):
        raise ValueError(f"target_kl={target_kl!r}: a positive finite number, or None")
    return v


def kl_stop(sums8, target_kl):
    """The early-stop rule after an epoch, from that epoch's eight (all-reduced) diagnostic sums (ops.PPO_DIAG_NAMES): stop when
    the epoch's mean k3 estimate  sums[1] / sums[7]  is greater than target_kl.  A plain comparison -- no 1.5 x factor as some
    other trainers apply, and a NaN estimate (NaN probabilities, which losses() reports) never stops."""
    return target_kl is not None and bool(float(sums8[1]) / float(sums8[7]) > target_kl)


def diagnostics_from_sums(sums, epochs_run=None, target_kl=None):
    """[epochs][8] per-epoch diagnostic sums (ops.PPO_DIAG_NAMES; an epoch's row = the sum over its optimiser steps, over all
    ranks) -> the dict VecPPOTrainer.diagnostics() returns: per-epoch lists over the epochs that ran of
      approx_kl            S1 / n   the k3 estimator, mean of expm1(lr) - lr   (what target_kl is compared with)
      approx_kl_k1         S0 / n   mean of logp_old - logp
      clip_fraction        S2 / n   samples whose ratio left [1 - clip, 1 + clip]
      value_clip_fraction  S3 / n   samples whose value moved more than clip from the rollout's
      explained_variance   1 - S4 / (S6 - S5^2 / n) = 1 - sum (R - V)^2 / sum (R - mean R)^2; NaN when the returns are constant
    and epochs_run, stopped_early.  epochs_run = None: the epochs are walked in order and the walk ends behind the first one that
    kl_stop() stops at -- the decision update() takes -- or at the first row without samples."""
    s = np.asarray(sums, dtype=np.float64).reshape(-1, 8)
    if epochs_run is None:
        epochs_run = 0
        for row in s:
            if not row[7] > 0:
                break
            epochs_run += 1
            if kl_stop(row, target_kl):
                break
    epochs_run = int(epochs_run)
    out = {k: [] for k in ("approx_kl", "approx_kl_k1", "clip_fraction", "value_clip_fraction", "explained_variance")}
    for S in s[:epochs_run]:
        n = S[7]
        out["approx_kl"].append(float(S[1] / n))
        out["approx_kl_k1"].append(float(S[0] / n))
        out["clip_fraction"].append(float(S[2] / n))
        out["value_clip_fraction"].append(float(S[3] / n))
        var_n = S[6] - S[5] * S[5] / n                       # n * variance of the returns
        # constant returns: S6 and S5^2 / n then agree up to the rounding of the f64 sums (about 1e-16 sqrt(n) relative), so a
        # difference below 1e-12 of the second moment is rounding, not variance
        out["explained_variance"].append(float(1.0 - S[4] / var_n) if var_n > 1e-12 * S[6] else float("nan"))
    out["epochs_run"] = epochs_run
    out["stopped_early"] = epochs_run < s.shape[0]
    return out


def _delegate(owner, name, setter=False):
    """A trainer attribute that lives on one of its collaborators (self.<owner>.<name>)."""
    def fset(self, v):
        setattr(getattr(self, owner), name, v)
    return property(lambda self: getattr(getattr(self, owner), name), fset if setter else None)


class VecPPOTrainer:
    def __init__(self, num_envs, horizon, policy="lstm", hidden=128, layers=1, variant="v2.0", device="cuda",
                 seed=1234, gae_mode="reference_exact", num_minibatches=1, bank=None, bank_sources=None,
                 rank=0, world_size=1, use_curriculum=True, trend_k=0, log_info=False, device_curriculum=None,
                 update_form="update_model", minibatch_rows=None, shuffle_envs=False, bptt_len=None, diagnostics=False,
                 target_kl=None, normalise_rewards=False, reward_clip=10.0, reward_norm_gamma=None, dgates_tile=None,
                 normalise_obs=False, obs_norm_eps=1e-4, obs_norm_channels=None, lr_schedule="constant", lr_final=None,
                 ent_beta_final=None, schedule_iterations=None, desired_kl=None, lr_factor=1.5, lr_min=1e-6, lr_max=1e-2,
                 eval_every=None, eval_envs=256, eval_seed=4321, eval_max_steps=None, eval_chunk=None, eval_radius=None, keep_best=True,
                 eval_source_fit=False, eval_source_stop=False, bank_truth=None, **hp):
        self.hp = dict(DEFAULTS)
        # eval_every: every so many iterations the policy runs one greedy episode on each of eval_envs envs of a separate, fixed
        # evaluation env (seed eval_seed, eval_radius or the env's default radius, eval_max_steps or the env's step limit, eval_chunk
        # steps per launch) and keep_best keeps the parameters of the best evaluation so far on the device, self.eval_tracker
        # (uavppo/eval_track.py).  No host read, and nothing training computes changes by a bit.  None: the iteration issues exactly
        # the launches it did without it.  eval_source_fit: False / None, True or a dict of check_source_fit's keywords: each
        # evaluation also estimates the plume's source from its records (uavppo/source_fit.py); the curve's rows gain "source".
        self.eval = check_eval(eval_every, eval_envs, eval_seed, eval_max_steps, eval_chunk, eval_radius, keep_best)
        # eval_source_fit={"model": "aniso"}: the six-term fit of plumes stretched along an axis (uavppo/source_aniso.py); bank_truth
        # f64 [F, 4] per field of `bank` (field_bank.load_with_truth) or None is what its widths, angle and peak are scored against.
        # It is read by that model only: training itself never sees it.
        self.eval["source_fit"] = source_fit_option(eval_source_fit)
        self.eval["bank_truth"] = bank_truth if (self.eval["source_fit"] or {}).get("model") == "aniso" else None
        # eval_source_stop: False / None, True or a dict of check_source_stop's keywords: the estimator also stops the evaluation's
        # episodes (uavppo/source_stop.py; implies eval_source_fit); the rows gain "stopped".  Set eval_radius small with it.
        self.eval["source_stop"] = source_stop_option(eval_source_stop)
        self.dgates_tile = dgates_tile       # gate gradients of the update in tile form: None = the rule of _request_dgates_tile, True / False = A/B
        self.hp.update(hp)
        # normalise_rewards: the GAE reads the reward scaled by a running estimate of the discounted return's standard deviation
        # and clamped to +-reward_clip (None: no clamp), self.reward_norm (uavppo/reward_norm.py); reward_norm_gamma: the discount of
        # that return, None = hp["gamma"].  buf["rew"] is never written.  Off: update() issues exactly the launches it did without it.
        self.normalise_rewards = bool(normalise_rewards)
        self.reward_clip, self.reward_norm_gamma = check_reward_norm(reward_clip, reward_norm_gamma, self.hp["gamma"])
        # normalise_obs: running per-channel observation statistics folded into the first layer, self.obs_norm (uavppo/obs_norm.py):
        # policy.flat holds the folded parameters, Adam updates the normaliser's master; obs_norm_channels: the channels that are
        # normalised (None: all).  buf["obs"] is never written.  Off: update() issues exactly the launches it did without it.
        self.normalise_obs, self.obs_norm_eps, self.obs_norm_mask = check_obs_norm(normalise_obs, obs_norm_eps, obs_norm_channels,
                                                                                   6 + int(trend_k))
        # diagnostics: every optimiser step's loss kernel also leaves eight sums (include/uavppo.h, uav_set_ppo_diag) that
        # update() adds up per epoch -- diagnostics() turns them into approx. KL, clip fractions and explained variance.
        # target_kl: after each epoch those sums are all-reduced and read (the update's one host wait per epoch) and the
        # remaining epochs are dropped once kl_stop() says so.  Both off: update() issues exactly the launches it did without them.
        self.target_kl = check_target_kl(target_kl)
        self.gae_mode, self.minibatch_rows, self._C = check_options(num_envs, horizon, policy, trend_k, update_form, gae_mode,
                                                                    num_minibatches, minibatch_rows, shuffle_envs, bptt_len)
        # lr_schedule / ent_beta_final (uavppo/lr_control.py): "linear" interpolates hp["lr"] -> lr_final over schedule_iterations
        # iterations, by value into the same Adam kernel; ent_beta_final does the same for the entropy weight under any schedule;
        # "adaptive" divides / multiplies the rate by lr_factor after an update whose last epoch's approx. KL left
        # [desired_kl / 2, 2 desired_kl], on the device (self.lr_control), and implies the diagnostics.  hp["lr"] and
        # hp["ent_beta"] stay the starting values.  "constant" without ent_beta_final: update() issues exactly the launches it did.
        rows = self.minibatch_rows
        steps = int(num_minibatches) if rows is None else -(-int(num_envs) * int(horizon) // rows)       # optimiser steps per epoch
        self.schedule = check_lr_control(lr_schedule, self.hp["lr"], lr_final, ent_beta_final, schedule_iterations, desired_kl,
                                         lr_factor, lr_min, lr_max, optimiser_steps=int(self.hp["epochs"]) * steps)
        self.lr_schedule = self.schedule["lr_schedule"]
        self._diag_on = bool(diagnostics) or self.target_kl is not None or self.lr_schedule == "adaptive"
        self.N, self.T = int(num_envs), int(horizon)
        self.rank, self.world = int(rank), int(world_size)
        self._coll = self.world > 1 or collectives_on()          # the three exchanges of an iteration are issued
        self.device = torch.device(device)
        self.variant, self.seed = variant, int(seed)
        self.update_form, self.num_minibatches, self.shuffle_envs = update_form, int(num_minibatches), bool(shuffle_envs)
        self.bptt_len = None if bptt_len is None else int(bptt_len)
        self.kind, self.trend_k = policy, int(trend_k)
        self.obs_dim = D = 6 + self.trend_k      # 6 reference features + trend channels (BASELINE C5)
        self._S, self._Ls = self.N * self._C, self.T // self._C       # the update's sequences: S rows of Ls steps (N, T without bptt_len)
        self._nb = self._S // self.num_minibatches                    # ... per minibatch
        self._last_n = self._nb * self._Ls                            # local samples of the last optimiser step (losses())
        self._env_lo = env_shard(self.rank, self.N)[0]                # environments of this rank: global indices [rank*N, (rank+1)*N)
        # the reference's MLP (256-128, 5 actions; 6 inputs, or 7 / 8 with the trend channels) has fused persistent kernels
        # (csrc/mlp_rollout.hip, csrc/mlp_update.hip); other sizes and fused_mlp=False take the layer-by-layer path (uav_mlp_fwd / uav_ppo_loss /
        # uav_mlp_bwd + step-wise rollout)
        self._fused_mlp = policy == "mlp" and 6 <= D <= 8
        self.reuse_rollout_forward = True    # epoch 0 adopts the rollout kernel's stash (same parameters)
        self.use_stepper = True              # h = 256 step-wise rollouts through uav_lstm_stepper_* (A/B switch)
        self.use_fused_tail = True           # ... and heads + sample + env step + store of a step as ONE launch (A/B switch)
        self._rollout_forward_valid = False
        self.record = False          # tests: keep (loss_sums, grad norm) of every optimiser step
        self.record_grads = False    # tests: ... and the (all-reduced, unclipped) flat gradient of every optimiser step + its parameters
        self.log = []
        self.grad_log = []
        self.forced_perms = None     # tests: list of index tensors [N * T] (shuffle_envs: [N], with bptt_len [N * C]), consumed in order instead of the drawn permutations
        self.perm_log = []           # tests (record, shuffle_envs): the env permutation of every epoch
        self._perm_gen = None        # device generator of the row / env permutations, seeded by (seed, rank) on first use
        self._iter_events = []       # (start, end) event pairs of time_rollouts() still to be recorded
        self._st = None              # scratch of one step of the step-wise rollouts: _step_scratch()
        self.opt_step = 0
        self.iteration = 0
        self._lr = self._ent_beta = None       # the values update() runs with, set at its top
        if policy == "lstm":
            self.policy = LSTMActorCritic(D, hidden, layers, 5, self.device, seed=self.seed)
        else:
            self.policy = MLPActorCritic(D, 5, device=self.device, seed=self.seed)
        # the allocation steps, in the order the tensors have always been allocated in
        self._alloc_samples(log_info)
        self._alloc_collaborators(bank, bank_sources, use_curriculum, device_curriculum)
        self._alloc_policy_work(hidden, layers)
        self._alloc_update_views(hidden, layers)
        self.reset()

    def _alloc_samples(self, log_info):
        """The [N][T] sample buffers a rollout fills, what GAE makes of them, and the optimiser's state."""
        N, T, D, d = self.N, self.T, self.obs_dim, self.device
        f32 = dict(dtype=torch.float32, device=d)
        self.buf = {"obs": torch.zeros(N, T, D, **f32), "act": torch.zeros(N, T, dtype=torch.int32, device=d),
                    "rew": torch.zeros(N, T, **f32), "val": torch.zeros(N, T, **f32), "logp": torch.zeros(N, T, **f32),
                    "done": torch.zeros(N, T, **f32), "flags": torch.zeros(N, T, dtype=torch.uint8, device=d),
                    "keep": torch.ones(N, T, **f32)}
        # optional per-step reward parts (for the reference's per-episode CSV columns, train_ppo2.0.py:129-135)
        self.info = torch.zeros(N, T, 10, **f32) if log_info else None    # reward parts | obs[2] | agent x, y | source x, y
        self.adv = torch.zeros(N, T, **f32)
        self.adv_n = torch.zeros(N, T, **f32)
        self.ret = torch.zeros(N, T, **f32)
        self.last_val = torch.zeros(N, **f32) if self.gae_mode in ("standard", "inline_v10") else None
        self.stats3 = torch.zeros(3, dtype=torch.float64, device=d)
        self.loss_sums = torch.zeros(4, dtype=torch.float64, device=d)
        self.gnorm = torch.zeros(1, **f32)
        self.dhead_bias = torch.zeros(6, **f32)
        self.nan_count = torch.zeros(1, dtype=torch.int32, device=d)
        P = self.policy.num_params()
        self.exp_avg = torch.zeros(P, **f32)
        self.exp_avg_sq = torch.zeros(P, **f32)
        # diagnostics: the buffer the loss kernels overwrite per call | its per-epoch sums of the last update() | the row in use
        self._diag_sums = torch.zeros(ops.PPO_DIAG_N, dtype=torch.float64, device=d) if self._diag_on else None
        self._diag_epochs = torch.zeros(int(self.hp["epochs"]), ops.PPO_DIAG_N, dtype=torch.float64, device=d) if self._diag_on else None
        self._diag_row = None
        self._diag_epochs_run = 0

    def _alloc_collaborators(self, bank, bank_sources, use_curriculum, device_curriculum):
        """The range guard, this rank's environments, and the curriculum link."""
        N, d = self.N, self.device
        self.guard = RangeGuard(self.policy, self.kind, d, enabled=self.kind == "lstm" or self._fused_mlp)
        self.env_state = torch.zeros(ops.env_state_bytes(N), dtype=torch.uint8, device=d)
        self.cur_obs = torch.zeros(N, self.obs_dim, dtype=torch.float32, device=d)
        self.bank = None if bank is None else torch.as_tensor(bank, dtype=torch.float64).to(d).contiguous()
        self.bank_sources = None if bank_sources is None else torch.as_tensor(bank_sources, dtype=torch.float64).to(d).contiguous()
        self.link = CurriculumLink(d, self.world, self._coll, use_curriculum, device_curriculum)
        self.reward_norm = (RewardNormaliser(N, self.T, self.reward_norm_gamma, self.reward_clip or None, device=d)
                            if self.normalise_rewards else None)
        self.obs_norm = ObsNormaliser(self.policy, self.kind, self.obs_norm_eps, self.obs_norm_mask, device=d) if self.normalise_obs else None
        sc = self.schedule
        self.lr_control = (LrController(self.hp["lr"], sc["desired_kl"], sc["lr_factor"], sc["lr_min"], sc["lr_max"], device=d)
                           if self.lr_schedule == "adaptive" else None)
        ev = self.eval
        self.eval_tracker = None
        if ev["eval_every"] is not None:
            self.eval_tracker = EvalTracker(self.policy, self.kind, ev["eval_envs"], self.variant, self.trend_k, ev["eval_seed"],
                                            self.bank, self.bank_sources, d, self.rank, self.world, ev["eval_max_steps"],
                                            ev["eval_chunk"], keep_best=ev["keep_best"], eval_radius=ev["eval_radius"],
                                            guard=self.guard, collectives=self._coll, source_fit=ev["source_fit"],
                                            source_stop=ev["source_stop"], bank_truth=ev["bank_truth"])

    def _alloc_policy_work(self, hidden, layers):
        """The recurrent state and the work arrays the update's kernels write their forward pass to."""
        N, nb, Ls = self.N, self._nb, self._Ls
        f32 = dict(dtype=torch.float32, device=self.device)
        if self.kind == "lstm":
            L, H = layers, hidden
            # recurrent state (h | c) and its snapshot at the start of the current rollout (what BPTT starts from): each pair is
            # ONE allocation, so the snapshot before a rollout is one copy launch instead of two
            self._state = torch.zeros(2, L, N, H, **f32)
            self._state0 = torch.zeros(2, L, N, H, **f32)
            self.h, self.c = self._state[0], self._state[1]
            self.h0, self.c0 = self._state0[0], self._state0[1]
            self.work = {"dgates": ops.lstm_dgates(nb, Ls, H, self.device), "heads": torch.empty(nb, Ls, 6, **f32)}   # heads: logits | value, written by the sequence kernels
            self._request_dgates_tile(L, H)
            for l in range(L):
                self.work[f"stash{l}"] = torch.empty(nb, Ls, 6 * H, **f32)
                self.work[f"y{l}"] = torch.empty(nb, Ls, H, **f32)
            # (a dy buffer for paths whose backward does not take dheads is allocated on first use: policy.backward)
            self.dhead_bias = self.policy.grad_views["head.bias"]       # the loss kernel's column sums ARE this gradient
        else:
            self.work = {"stash": None}      # layer-by-layer path only (770 floats per sample); allocated on first use
            self._step_scratch()
        self.dheads = torch.empty(nb * Ls, 6, **f32)

    def _request_dgates_tile(self, layers, hidden):
        """Whether this trainer's own work["dgates"] is written and read in TILE form (include/uavppo.h, uav_lstm_dgates_tile: the
        16 rows a BPTT workgroup writes per step adjacent instead of Ls rows apart; same values, same gradients to the bit).  The
        request is made per uav_lstm_bwd call for this one buffer (ops.lstm_bwd, dgates_tile="transient"), never as a mode of the
        device handle, which everything on the device shares.  Asked for when the form exists for the shape -- one layer,
        h = 64 / 128, at most 6 inputs, sequences of a multiple of 32 steps; the library has the last word
        (ops.lstm_dgates_tile_bytes) -- and when it pays: the form helps the BPTT where HBM binds it, which takes a
        16-env tile on every CU.  Rule: tiles = ceil(nb / 16) >= the device's CU count.  Evidence
        (profiles/dgates_tile_perf.json; one MI355X, 256 CUs, parent and this tree alternating): C3, 256 tiles: the BPTT 0.548-0.555
        -> 0.527-0.529 ms per launch, the weight-gradient pass unchanged, the iteration 6.72-6.82 -> 6.58-6.68 ms; C4, 64 tiles:
        4.348-4.351 ms on rows, 4.373-4.383 with the form forced (slower); C2, 16 tiles: 1.482-1.485 against 1.480-1.483 (nothing).
        Tile counts between 64 and 256 are not measured and keep rows.  dgates_tile=True / False, or UAVPPO_DGATES_TILE=1 / 0 in the
        environment of a caller that cannot pass it, override the rule for A/B runs (the shape conditions still hold)."""
        self.policy.dgates_tile = False
        want = self.dgates_tile
        if os.environ.get("UAVPPO_DGATES_TILE") in ("0", "1"):         # A/B runs of unchanged callers (bench.py)
            want = os.environ["UAVPPO_DGATES_TILE"] == "1"
        if want is False or layers != 1 or hidden not in (64, 128) or self.obs_dim > 6 or self._Ls % 32:
            return
        if want is None and (self._nb + 15) // 16 < torch.cuda.get_device_properties(self.device).multi_processor_count:
            return
        nbytes = ops.lstm_dgates_tile_bytes(self._nb, self._Ls, self.obs_dim, hidden, self.device)
        if not nbytes:
            return
        if self.work["dgates"].numel() * 4 < nbytes:                   # nb is no multiple of 16: the last tile is padded
            self.work["dgates"] = torch.empty(nbytes // 4, dtype=torch.float32, device=self.device)
        self.policy.dgates_tile = True

    def _alloc_update_views(self, hidden, layers):
        """What the update reads its sequences from: the sample arrays and the start state themselves, or -- truncated BPTT --
        their [N * C][Lc] views and the chunks' start states h0c, c0c [L][N * C][H]; with shuffle_envs, the packed minibatch."""
        N, T, d, nb, S, Ls = self.N, self.T, self.device, self._nb, self._S, self._Ls
        f32 = dict(dtype=torch.float32, device=d)
        lstm = self.kind == "lstm"
        self._u = {"obs": self.buf["obs"], "act": self.buf["act"], "logp": self.buf["logp"], "val": self.buf["val"],
                   "keep": self.buf["keep"], "adv_n": self.adv_n, "ret": self.ret}
        self._rwork = self.work                # the [N][T] arrays a rollout writes its forward pass to (epoch 0 adopts it)
        if lstm:
            self._u["h0"], self._u["c0"] = self.h0, self.c0
        if self._C > 1:
            self._u = {k: v.view((S, Ls) + tuple(v.shape[2:])) for k, v in self._u.items() if k not in ("h0", "c0")}
            self.h0c, self.c0c = torch.zeros(layers, S, hidden, **f32), torch.zeros(layers, S, hidden, **f32)
            self._u["h0"], self._u["c0"] = self.h0c, self.c0c
            if self.num_minibatches == 1:      # one minibatch: the work arrays hold all N * T samples, chunk rows in buffer order
                self._rwork = {k: v.view(N, T, -1) for k, v in self.work.items() if k != "dgates"}
        self._pack = self._pack_plan = None
        if self.shuffle_envs:
            # the packed minibatch: nb whole env sequences of the seven sample arrays (the MLP: six, it has no restart mask) and
            # the LSTM's start state, allocated once; the plan holds the checked (source, destination) table of the launch
            u, pk = self._u, {}
            src = {k: u[k] for k in ("obs", "act", "logp", "adv_n", "ret", "val")}
            if lstm:
                src["keep"] = u["keep"]
            for k, v in src.items():
                pk[k] = torch.empty((nb,) + tuple(v.shape[1:]), dtype=v.dtype, device=d)
            pairs = [(src[k], pk[k]) for k in src]
            if lstm:
                pk["h0"], pk["c0"] = torch.empty(layers, nb, hidden, **f32), torch.empty(layers, nb, hidden, **f32)
                pairs += [(u["h0"], pk["h0"], 1), (u["c0"], pk["c0"], 1)]
            self._pack, self._pack_plan = pk, ops.GatherPlan(pairs)

    # ------------------------------------------------------------------------------------------
    def env_cfg(self):
        k = self.link
        return ops.make_env_cfg(self.variant, k.host_radius, k.host_bonus, self.seed, self.bank, self.bank_sources,
                                env_offset=self._env_lo, n_env_total=self.world * self.N,
                                trend_k=self.trend_k, curriculum=k.block)

    # ------------------------------------------------------------------------------------------ the two collaborators' surface
    # T1, successes -> curriculum: self.link (uavppo/curriculum_link.py).  The getters of radius / bonus / episodes_done /
    # successes_done WAIT for a device curriculum; the training loop reads the lagged ones.
    curriculum = _delegate("link", "curriculum")
    device_curriculum = _delegate("link", "device_curriculum")
    last_mirror_slot = _delegate("link", "last_mirror_slot")
    last_success_bits = _delegate("link", "last_success_bits")
    side_stream_curriculum = _delegate("link", "use_side_stream", setter=True)
    radius = _delegate("link", "radius", setter=True)
    bonus = _delegate("link", "bonus", setter=True)
    radius_lagged = _delegate("link", "radius_lagged")
    episodes_lagged = _delegate("link", "episodes_lagged")
    episodes_done = _delegate("link", "episodes_done")
    successes_done = _delegate("link", "successes_done")

    def rollout_radius(self, k=None):
        return self.link.rollout_radius(k)

    def episodes_before_rollout(self, k):
        return self.link.episodes_before_rollout(k)

    def sync_curriculum(self):
        return self.link.sync()

    def update_curriculum(self):
        return self.link.count(self.buf["flags"])

    # range guard: self.guard (uavppo/range_guard.py)
    arith = _delegate("guard", "arith")
    range_events = _delegate("guard", "range_events")
    force_arith = _delegate("guard", "force_arith", setter=True)

    def poll_param_range(self):
        return self.guard.poll()

    def check_ranges(self):
        return self.guard.before_update(self.buf["obs"], self.h0 if self.kind == "lstm" else None)

    @property
    def fused_mlp(self):
        return self._fused_mlp

    @fused_mlp.setter
    def fused_mlp(self, on):             # (A/B, tests: False sends a fused-size MLP down the layer-by-layer path, which has no guard)
        self._fused_mlp = bool(on)
        self.guard.enabled = self.kind == "lstm" or self._fused_mlp

    def reset(self):
        ops.env_reset(self.env_state, self.N, self.env_cfg(), self.cur_obs)
        if self.kind == "lstm":
            self.h.zero_()
            self.c.zero_()
        if self.reward_norm is not None:
            self.reward_norm.reset()
        if self.obs_norm is not None:
            self.obs_norm.reset()
        if self.lr_control is not None:
            self.lr_control.reset(self.hp["lr"])

    # ------------------------------------------------------------------------------------------ R1
    def _stepwise_lstm_route(self):
        """h = 256 on the fp16-split arithmetic, one minibatch: the stepper (uav_lstm_stepper_*) -- weights split once per
        rollout, state kept in its piece planes, stash / y / heads written at [:, t] of the update's own arrays, so that
        PPO epoch 0 adopts this forward pass -- with everything after the recurrent layers as one launch (uav_rollout_tail)
        unless the per-step info rows are wanted.  Otherwise one uav_lstm_fwd call of T = 1 per layer and step."""
        if not (self.use_stepper and self.policy.hidden == 256 and self.arith == "fp16x3" and self.num_minibatches == 1
                and ops.lstm_bwd_caps(self.device, self.obs_dim, 256) != 0):      # 0: the handle is not on the fp16 step path
            return "per_call"
        return "tail" if self.use_fused_tail and self.info is None else "stepper"

    def rollout_route(self):
        """Which rollout the next collect() runs on the arithmetic in force: 'fused_lstm' | 'fused_mlp' (uav_rollout, one
        persistent launch), or step-wise 'tail' | 'stepper' | 'per_call' (LSTM), 'per_call' (MLP)."""
        if self.kind != "lstm":
            return "fused_mlp" if self.fused_mlp else "per_call"
        wide = self.guard.enabled and self.arith != "fp16x3"     # uav_rollout exists in the fp16-split form only
        if self.policy.num_layers == 1 and self.policy.hidden in (64, 128) and not wide:
            return "fused_lstm"
        return self._stepwise_lstm_route()

    def collect(self, forced_act=None, noise=None):
        """Fill the (env, T, feat) buffers with one rollout of T steps per env."""
        self._rollout_forward_valid = False
        self.link.before_rollout()
        self.guard.before_rollout()
        route = self.rollout_route()
        if self.kind == "lstm":
            self._state0.copy_(self._state)
        if route == "fused_lstm":
            reuse = self.reuse_rollout_forward and self.num_minibatches == 1
            ops.rollout_lstm(self.env_state, self.N, self.env_cfg(), self.policy.flat, self.policy.hidden, self.T,
                             self.iteration, self.cur_obs, self.h[0], self.c[0], self.buf, last_val=self.last_val,
                             forced_act=forced_act, noise=noise, nan_count=self.nan_count,
                             stash=self._rwork["stash0"] if reuse else None, y=self._rwork["y0"] if reuse else None,
                             info=self.info, heads=self._rwork["heads"] if reuse else None)
            self._rollout_forward_valid = reuse
        elif route == "fused_mlp":
            ops.rollout_mlp(self.env_state, self.N, self.env_cfg(), self.policy.flat, self.T, self.iteration, self.cur_obs,
                            self.buf, last_val=self.last_val, forced_act=forced_act, noise=noise, nan_count=self.nan_count,
                            info=self.info, trend=self.trend_k != 0)
        elif self.kind == "lstm":
            self._collect_stepwise_lstm(forced_act, noise)
        else:
            self._collect_stepwise(forced_act, noise)
        self.link.after_rollout(self.buf["flags"])

    def _step_scratch(self):
        """Scratch of ONE step of the step-wise rollouts (every route but the two fused kernels), built once -- an LSTM's on its
        first step-wise rollout: what the env step returns, the per-call routes' forward stashes, the action drawn and the restart
        mask carried to the next step (LSTM), and -- with log_info -- the step's reward parts, terminal observation and source."""
        if self._st is None:
            N, d, log, f32 = self.N, self.device, self.info is not None, dict(dtype=torch.float32, device=self.device)
            self._st = {"rew": torch.zeros(N, **f32), "done": torch.zeros(N, **f32), "flags": torch.zeros(N, dtype=torch.uint8, device=d),
                        "work": {}, "stash": None, "info": torch.zeros(N, 5, **f32) if log else None,
                        "term": torch.zeros(N, self.obs_dim, **f32) if log else None,
                        "src": torch.zeros(N, 2, dtype=torch.float64, device=d) if log else None}
            if self.kind == "lstm":
                self._st.update(act=torch.zeros(N, dtype=torch.int32, device=d), keep=torch.ones(N, **f32))
        return self._st

    def _env_step(self, st, cfg, act, t, noise):
        """Env step t of a step-wise rollout into the step scratch; with log_info, row t of the ten info columns."""
        nz = None if noise is None else noise[:, t].contiguous()
        if self.info is not None:
            ops.env_peek(self.env_state, self.N, source=st["src"])           # source of the episode this step belongs to
        ops.env_step(self.env_state, self.N, cfg, act, self.cur_obs, st["rew"], st["done"], st["flags"], noise=nz,
                     info=st["info"], term_obs=st["term"])
        if self.info is not None:
            self.info[:, t, :5] = st["info"]
            self.info[:, t, 5] = st["term"][:, 2]
            self.info[:, t, 6:8] = st["term"][:, :2] * 500.0       # step-wise path: position from the observation
            self.info[:, t, 8:10] = st["src"]

    def _rollout_per_call(self, heads_of, forced_act, noise, keep=None):
        """One policy forward + sample + env step launch group per time step (train_ppo2.0.py:157-198 with a batch of N states
        instead of 1).  heads_of(): logits | value [N, 6] of the current observation; keep: the LSTM's restart mask [N]."""
        b, st, cfg = self.buf, self._step_scratch(), self.env_cfg()
        for t in range(self.T):
            heads = heads_of()
            fa = None if forced_act is None else forced_act[:, t].contiguous()
            act, logp, _, _ = ops.policy_sample(heads[:, :5].contiguous(), seed=self.seed, counter=t, iteration=self.iteration,
                                                index_offset=self._env_lo, forced_act=fa, nan_count=self.nan_count)
            b["obs"][:, t] = self.cur_obs
            b["act"][:, t] = act
            b["val"][:, t] = heads[:, 5]
            b["logp"][:, t] = logp
            if keep is not None:
                b["keep"][:, t] = keep
            self._env_step(st, cfg, act, t, noise)
            b["rew"][:, t] = st["rew"]
            b["done"][:, t] = st["done"]
            b["flags"][:, t] = st["flags"]
            if keep is not None:
                torch.sub(1.0, st["done"], out=keep)      # the recurrent state restarts where an episode ended

    def _rollout_stepper(self, forced_act, noise):
        b, st, w, cfg = self.buf, self._st, self._rwork, self.env_cfg()
        for t in range(self.T):
            b["obs"][:, t] = self.cur_obs
            self.policy.step_at(b["obs"], t, w, w["heads"], keep=st["keep"])
            fa = None if forced_act is None else forced_act[:, t].contiguous()
            # sample from heads[:, t] in place; action / value / log-prob straight into column t
            act = ops.policy_sample_at(w["heads"], t, st["act"], b["act"], b["val"], b["logp"], self.nan_count, seed=self.seed,
                                       iteration=self.iteration, index_offset=self._env_lo, forced_act=fa)
            self._env_step(st, cfg, act, t, noise)
            # one launch: keep / rew / done / flags -> column t; keep <- 1 - done
            ops.store_transition(t, st["keep"], st["rew"], st["done"], st["flags"], b["keep"], b["rew"], b["done"], b["flags"])

    def _rollout_tail(self, forced_act, noise):
        b, st, w, cfg, v = self.buf, self._st, self._rwork, self.env_cfg(), self.policy.views
        b["obs"][:, 0] = self.cur_obs                  # later rows are written by the tail of the step before
        for t in range(self.T):
            top = self.policy.step_layers_at(b["obs"], t, w, keep=st["keep"])
            ops.rollout_tail(self.env_state, cfg, top, t, v["head.weight"], v["head.bias"], w["heads"], st["act"],
                             self.cur_obs, b["obs"], st["keep"], b["act"], b["val"], b["logp"], b["keep"], b["rew"], b["done"],
                             b["flags"], self.nan_count, seed=self.seed, iteration=self.iteration, index_offset=self._env_lo,
                             forced_act=None if forced_act is None else forced_act[:, t].contiguous(),
                             noise=None if noise is None else noise[:, t].contiguous())

    def _collect_stepwise_lstm(self, forced_act=None, noise=None):
        """Stacked / wide LSTM policies (BASELINE C5: h=256 x2) on the step-wise route this trainer's switches select.  Same
        buffers and keep semantics as the fused rollout kernel.  (The caller snapshots _state0.)"""
        st, route = self._step_scratch(), self._stepwise_lstm_route()
        st["keep"].fill_(1.0)
        if route == "per_call":
            self._rollout_per_call(lambda: self.policy.step(self.cur_obs, self.h, self.c, st["keep"], st["work"]), forced_act, noise,
                                   keep=st["keep"])
        else:
            self.policy.begin_steps(self.h, self.c)
            (self._rollout_tail if route == "tail" else self._rollout_stepper)(forced_act, noise)
            for l, sp in enumerate(self.policy.steppers(self.N, self.device)):
                self.h[l].copy_(sp.hn)
                self.c[l].copy_(sp.cn)
            self._rollout_forward_valid = self.reuse_rollout_forward
        # hand the state to the next rollout already masked (its keep[:, 0] is 1), like the fused kernel
        self.h.mul_(st["keep"][None, :, None])
        self.c.mul_(st["keep"][None, :, None])
        if self.last_val is not None:
            hh, cc = self.h.clone(), self.c.clone()
            self.last_val.copy_(self.policy.step(self.cur_obs, hh, cc, None, st["work"])[:, 5])

    def _collect_stepwise(self, forced_act=None, noise=None):
        """MLP policy on the layer-by-layer kernels (uav_mlp_fwd), the forward stash kept across steps."""
        st = self._step_scratch()

        def heads_of():
            heads = self.policy.heads(self.cur_obs, stash=st["stash"])
            st["stash"] = self.policy._stash
            return heads
        self._rollout_per_call(heads_of, forced_act, noise)
        if self.last_val is not None:
            self.last_val.copy_(heads_of()[:, 5])

    # ------------------------------------------------------------------------------------------ G1, G2
    def _gae_reward(self):
        """The reward array the GAE reads (GAILTrainer: the shaped reward)."""
        return self.buf["rew"]

    def compute_advantages(self):
        b, hp = self.buf, self.hp
        rew = self._gae_reward()
        if self.reward_norm is not None:          # N1-N3: the scaled copy rew_n; the array it reads stays as it is.  Every call
            # takes the buffers into the running estimate as one more rollout (update() makes the call: once per rollout)
            rew = self.reward_norm(rew, b["done"])
        ops.gae(rew, b["val"], b["done"], hp["gamma"], hp["lam"], self.gae_mode, last_val=self.last_val, out=self.adv)
        ops.adv_stats(self.adv, out=self.stats3)
        allreduce_adv_stats(self.stats3)          # (sum, sumsq, count): whole-buffer statistics over all ranks
        normalise = ops.adv_normalise_inline if self.update_form == "inline_v10" else ops.adv_normalise
        normalise(self.adv, b["val"], self.stats3, self.adv_n, self.ret)

    # ------------------------------------------------------------------------------------------ U1-U3
    # minibatch slice -> flat gradient, one routine per policy kind (loss: the arguments of the loss kernel after the heads)
    def _grad_lstm(self, sl, loss, pk=None):
        u, M = self._u, self.num_minibatches
        if self._rollout_forward_valid:
            # first optimiser step after a fused rollout: parameters unchanged since the rollout, whose
            # kernel already wrote this forward pass (stash, y) and its heads (truncated BPTT: seen through the chunk view)
            L = self.policy.num_layers
            self.policy.adopt_forward(u["obs"], u["keep"], u["h0"], [self.work[f"stash{l}"] for l in range(L)],
                                      [self.work[f"y{l}"] for l in range(L)])
            heads = self.work["heads"]
            self._rollout_forward_valid = False
        elif pk is not None:             # a packed minibatch of shuffled envs: its own start state beside it
            heads = self.policy.heads(pk["obs"], pk["keep"], pk["h0"], pk["c0"], self.work)
        else:
            heads = self.policy.heads(u["obs"][sl], u["keep"][sl], u["h0"][:, sl].contiguous() if M > 1 else u["h0"],
                                      u["c0"][:, sl].contiguous() if M > 1 else u["c0"], self.work)
        ops.ppo_loss_heads(heads.view(self.dheads.shape[0], -1), *loss)
        return self.policy.backward(self.dheads, self.work, self.dhead_bias)

    def _grad_fused_mlp(self, sl, loss, pk=None):
        obs = (self.buf["obs"][sl] if pk is None else pk["obs"]).reshape(-1, self.obs_dim)
        if self.trend_k:
            return ops.mlp_ppo_grad_trend(self.policy.flat, obs, *loss[:8], self.loss_sums, self.policy.grad, self.trend_k)
        return ops.mlp_ppo_grad(self.policy.flat, obs, *loss[:8], self.loss_sums, self.policy.grad)

    def _grad_layered_mlp(self, sl, loss, pk=None):
        n = self.dheads.shape[0]
        if self.work["stash"] is None:
            self.work["stash"] = torch.empty(n * (2 * 256 + 2 * 128 + 2), dtype=torch.float32, device=self.device)
        heads = self.policy.heads((self.buf["obs"][sl] if pk is None else pk["obs"]).reshape(n, self.obs_dim), stash=self.work["stash"])
        ops.ppo_loss_heads(heads, *loss)
        return self.policy.backward(self.dheads)

    def _next_perm(self):
        """One permutation of this rank's N * T sample rows (row = env * T + t) -- with shuffle_envs of its N envs, or with
        bptt_len beside it of its N * C chunk rows -- as i32 on the device."""
        L = self._S if self.shuffle_envs else self.N * self.T
        if self.forced_perms is not None:
            perm = torch.as_tensor(self.forced_perms.pop(0)).to(self.device).reshape(-1)
            if perm.numel() != L:
                raise ValueError(f"forced_perms: a permutation of {perm.numel()} rows for a buffer of {L}")
        else:
            if self._perm_gen is None:
                self._perm_gen = torch.Generator(device=self.device).manual_seed(self.seed * 1000003 + self.rank)
            perm = torch.randperm(L, generator=self._perm_gen, device=self.device)
        return perm.to(torch.int32)

    def _optimiser_step(self, grad):
        hp = self.hp
        if self._diag_row is not None:   # diagnostics: this step's eight sums (its loss kernel just wrote them) into the epoch's row
            self._diag_row.add_(self._diag_sums)
        allreduce_grad(grad)              # RCCL sum over ranks; inv_n already holds 1/global count
        on, params = self.obs_norm, self.policy.flat
        if on is not None:               # the gradient and the parameters Adam sees are the master's (clip norm and moments too)
            on.unfold_grad(grad)
            params = on.master
        if self.record_grads:            # (gradient, parameters it was taken at)
            self.grad_log.append((grad.clone(), params.clone()))
        self.opt_step += 1
        if self.lr_control is not None:  # the rate the last update's KL left on the device; never read here
            ops.clip_adam_dlr(params, grad, self.exp_avg, self.exp_avg_sq, self.opt_step, self.lr_control.lr_dev,
                              max_norm=hp["max_grad_norm"], gnorm_out=self.gnorm, pmax_out=self.guard.ranges[0:1])
        else:
            ops.clip_adam(params, grad, self.exp_avg, self.exp_avg_sq, self.opt_step, self._lr,
                          max_norm=hp["max_grad_norm"], gnorm_out=self.gnorm, pmax_out=self.guard.ranges[0:1])
        if on is not None:               # policy.flat <- fold(master); the guard's slot raised to max |policy.flat|
            on.fold(self.guard.ranges[0:1])
        if self.record:
            self.log.append((self.loss_sums.clone(), self.gnorm.clone()))

    def _epoch_rows(self):
        """One epoch in shuffled row minibatches: every rank cuts its own permutation into the same number of chunks, so the
        gradient all-reduces pair up; inv_n = 1 / (len(chunk) * world)."""
        b, hp = self.buf, self.hp
        flat = [b["obs"].view(-1, self.obs_dim)] + [x.view(-1) for x in (b["act"], b["logp"], self.adv_n, self.ret, b["val"])]
        for rows in self._next_perm().split(self.minibatch_rows):
            self._last_n = rows.numel()
            grad = ops.mlp_ppo_grad_rows(self.policy.flat, *flat, rows.contiguous(), 1.0 / float(rows.numel() * self.world),
                                         hp["clip"], self._ent_beta, self.loss_sums, self.policy.grad, self.trend_k)
            self._optimiser_step(grad)

    def _epoch_envs(self, grad_of, inv_n):
        """One epoch in shuffled minibatches of whole env sequences: every rank cuts its own permutation of its N envs into the
        same num_minibatches chunks of N / M, so the gradient all-reduces pair up; a chunk is packed by one launch and then
        takes the unshuffled minibatch's route through grad_of and the optimiser step."""
        hp, pk, nb = self.hp, self._pack, self._nb
        perm = self._next_perm()
        if self.record:
            self.perm_log.append(perm)
        loss = (pk["act"].view(-1), pk["logp"].view(-1), pk["adv_n"].view(-1), pk["ret"].view(-1), pk["val"].view(-1), inv_n,
                hp["clip"], self._ent_beta, self.loss_sums, self.dheads, self.dhead_bias)
        for m in range(self.num_minibatches):
            ops.gather_rows_multi(perm[m * nb:(m + 1) * nb], self._pack_plan)
            self._optimiser_step(grad_of(None, loss, pk))

    def _chunk_start_states(self):
        """Truncated BPTT: h0c, c0c [L][N * C][H], the state every chunk row starts from, with the parameters as they are before
        the iteration's first optimiser step -- the rollout's -- and fixed for all its epochs.  Taken from the rollout's own
        forward pass where epoch 0 is about to adopt it; otherwise from ONE forward pass over the buffers, run in env slices
        that fit the update's work arrays, which the first optimiser step overwrites."""
        b, L, Lc, C = self.buf, self.policy.num_layers, self._Ls, self._C
        if self._rollout_forward_valid:
            w = self._rwork
            for l in range(L):
                ops.lstm_chunk_states(w[f"y{l}"], w[f"stash{l}"], b["keep"], self.h0[l], self.c0[l], Lc, self.h0c[l], self.c0c[l])
            return
        ns = max(1, (self._nb * Lc) // self.T)             # whole env sequences the work arrays of one minibatch hold
        for e0 in range(0, self.N, ns):
            e1 = min(e0 + ns, self.N)
            n, whole = e1 - e0, e0 == 0 and e1 == self.N
            w = {}
            if n * self.T <= self._nb * Lc:
                for l in range(L):
                    for k in (f"stash{l}", f"y{l}"):
                        a = self.work[k]
                        w[k] = a.view(-1)[:n * self.T * a.shape[2]].view(n, self.T, a.shape[2])
            h0, c0 = (self.h0, self.c0) if whole else (self.h0[:, e0:e1].contiguous(), self.c0[:, e0:e1].contiguous())
            keep = b["keep"][e0:e1]
            self.policy.heads(b["obs"][e0:e1], keep, h0, c0, w, want_heads=False)
            for l, (_, stash, y, _) in enumerate(self.policy._saved[0]):
                ops.lstm_chunk_states(y, stash, keep, h0[l], c0[l], Lc, self.h0c[l, e0 * C:e1 * C], self.c0c[l, e0 * C:e1 * C])
            self.policy._saved = None

    def update(self):
        """GAE + EPOCHS x num_minibatches optimiser steps (_update_model, train_ppo2.0.py:15-88) -- with shuffle_envs over a
        fresh permutation of the envs per epoch -- or with minibatch_rows EPOCHS x ceil(N T / minibatch_rows) steps over
        shuffled rows.  With diagnostics / target_kl the epochs run under _epochs_with_diagnostics, which may end them early."""
        if self.check_ranges() != "fp16x3":
            self._rollout_forward_valid = False
        # this iteration's step size and entropy weight, for all its steps (adaptive: the rate stays on the device, unread)
        self._lr = None if self.lr_control is not None else self.learning_rate()
        self._ent_beta = self.entropy_beta()
        self.compute_advantages()
        self.link.in_update()             # (the success exchange, behind the advantage-statistics all-reduce)
        u, hp = self._u, self.hp
        nb = self._nb
        inv_n = 1.0 / float(nb * self._Ls * self.world)
        if self._C > 1:
            self._chunk_start_states()
        grad_of = self._grad_lstm if self.kind == "lstm" else self._grad_fused_mlp if self.fused_mlp else self._grad_layered_mlp

        def epoch():
            if self.minibatch_rows is not None:
                return self._epoch_rows()
            if self.shuffle_envs:
                return self._epoch_envs(grad_of, inv_n)
            for m in range(self.num_minibatches):
                sl = slice(m * nb, (m + 1) * nb)
                grad = grad_of(sl, (u["act"][sl].reshape(-1), u["logp"][sl].reshape(-1), u["adv_n"][sl].reshape(-1),
                                    u["ret"][sl].reshape(-1), u["val"][sl].reshape(-1), inv_n, hp["clip"], self._ent_beta,
                                    self.loss_sums, self.dheads, self.dhead_bias))
                self._optimiser_step(grad)

        if not self._diag_on:
            for _ in range(hp["epochs"]):
                epoch()
        else:
            self._epochs_with_diagnostics(epoch, int(hp["epochs"]))
        if self.obs_norm is not None:     # this rollout's observations into the statistics the NEXT rollout and update run on
            self.obs_norm.after_update(self.buf["obs"], self.guard.ranges[0:1])
        self.guard.after_update()
        return self.loss_sums

    def _epochs_with_diagnostics(self, epoch, epochs):
        """update()'s epochs with the diagnostics buffer attached to the device's handle -- for their duration only: whatever else
        uses the handle (the discriminator steps, a caller's own loss calls) never sees it.  Row e of _diag_epochs collects
        epoch e's sums.  With target_kl the row is all-reduced and read after the epoch and kl_stop() decides whether the next
        one runs: the decision is a function of the all-reduced row alone, which every rank holds identically, so the ranks
        leave the loop together (a rank that stopped alone would leave the others waiting in the next gradient all-reduce).
        Without target_kl the whole array is all-reduced once, behind the last epoch, and nothing is read."""
        if self._diag_epochs.shape[0] != epochs:
            self._diag_epochs = torch.zeros(epochs, ops.PPO_DIAG_N, dtype=torch.float64, device=self.device)
        self._diag_epochs.zero_()
        self._diag_epochs_run = 0
        ops.set_ppo_diag(self._diag_sums, self.device)
        try:
            for e in range(epochs):
                self._diag_row = self._diag_epochs[e]
                epoch()
                self._diag_epochs_run = e + 1
                if self.target_kl is not None:
                    if self._coll:
                        allreduce_sum(self._diag_row)
                    if kl_stop(self._diag_row.cpu().numpy(), self.target_kl):
                        break
        finally:
            self._diag_row = None
            ops.set_ppo_diag(None, self.device)
        if self.target_kl is None and self._coll:
            allreduce_sum(self._diag_epochs)
        if self.lr_control is not None:   # once per update, behind the all-reduce of the row it reads: the next update's rate
            self.lr_control.adapt(self._diag_epochs[self._diag_epochs_run - 1])

    def diagnostics(self):
        """The last update()'s per-epoch diagnostics (diagnostics_from_sums: approx_kl, approx_kl_k1, clip_fraction,
        value_clip_fraction, explained_variance as lists over the epochs that ran; epochs_run; stopped_early), over all ranks'
        samples.  One host read; no collective (update() issued it)."""
        if not self._diag_on:
            raise RuntimeError("diagnostics(): build the trainer with diagnostics=True (or a target_kl)")
        return diagnostics_from_sums(self._diag_epochs.cpu().numpy(), epochs_run=self._diag_epochs_run)

    def learning_rate(self):
        """The step size the NEXT update() runs with: hp["lr"], its linear interpolation at self.iteration, or -- adaptive -- the
        controller's rate, which is a host read (for logs, not for the loop: update() never calls it then)."""
        sc = self.schedule
        if self.lr_control is not None:
            return self.lr_control.lr()
        if self.lr_schedule == "linear":
            return float(linear_value(self.hp["lr"], sc["lr_final"], self.iteration, sc["schedule_iterations"]))
        return self.hp["lr"]

    def entropy_beta(self):
        """The entropy weight the NEXT update() runs with: hp["ent_beta"], or its linear interpolation at self.iteration."""
        sc = self.schedule
        if sc["ent_beta_final"] is None:
            return self.hp["ent_beta"]
        return float(linear_value(self.hp["ent_beta"], sc["ent_beta_final"], self.iteration, sc["schedule_iterations"]))

    def time_rollouts(self, event_pairs):
        """Measurement hook (bench.py): the next len(event_pairs) calls of train_iteration() record a (start, end) pair of
        torch.cuda.Event around their rollout on the current stream -- the loop that is timed stays train_iteration() itself."""
        self._iter_events = list(event_pairs)[::-1]

    def _after_update(self):
        """Between update() and update_curriculum() of an iteration (GAILTrainer: the discriminator steps)."""

    def evaluate_if_due(self):
        """The in-training greedy evaluation (eval_every), at the end of an iteration: after self.iteration was advanced, so the
        evaluation tagged k sees the parameters after k updates.  The scripts' loops call it where train_iteration() does."""
        if self.eval_tracker is not None and self.iteration % self.eval["eval_every"] == 0:
            self.eval_tracker.run(self.iteration)

    def train_iteration(self):
        ev = self._iter_events.pop() if self._iter_events else None
        if ev is not None:
            ev[0].record()
        self.collect()
        if ev is not None:
            ev[1].record()
        sums = self.update()
        self._after_update()
        self.update_curriculum()
        self.poll_param_range()
        self.iteration += 1
        self.evaluate_if_due()
        return sums

    def losses(self):
        """(policy_loss, value_loss, entropy) of the LAST optimiser step; raises on NaN probabilities
        like the reference (train_ppo2.0.py:58-62)."""
        # the rollout's NaN counter travels with the loss sums, so EVERY rank sees every rank's count and they all
        # raise together (a rank raising alone would leave the others waiting in the next all-reduce)
        t = torch.cat([self.loss_sums, self.nan_count.to(torch.float64)])
        if self._coll:
            allreduce_sum(t)
        s = t.cpu().numpy()
        if s[3] > 0 or s[4] > 0:
            raise RuntimeError("NaN in probs")
        n = self._last_n * self.world           # (row minibatches: the last chunk's size, the same on every rank)
        return s[0] / n, s[1] / n, s[2] / n
