"""Behaviour cloning: supervised training of a policy on expert (state, action) pairs (generate_expert_data.py) with the
fused loss kernels uav_bc_loss / uav_mlp_bc_grad.  The reference has no such step -- its expert data feed the GAIL
discriminator only; cloning is what comes before GAIL or PPO fine-tuning, and what moves a trained policy into another
architecture (an h = 256 x 2 LSTM into a policy the fused rollout and greedy kernels cover).

The loss of one optimiser step over its unmasked samples (csrc/loss_core.h: bc_sample):
    total = mean(-log q[a]) + value_coef * mean(0.5 (V - R)^2) - ent_beta * mean(H)
with q the clamped Categorical probability and H the entropy of the PPO loss.  A sample whose action is outside 0 .. 4 is
masked: the padded steps of ragged episodes carry action -1.

Routes of BCTrainer, one optimiser step per chunk of a shuffled epoch:
    fused-size MLP (6+k-256-128)   ops.mlp_bc_grad(rows=chunk) on the resident expert set, no gather
    other MLP sizes                index_select, heads() + ops.bc_loss_heads + backward()
    LSTM                           chunks of whole episodes, padded to the longest: heads() from a zero state with keep = 1,
                                   ops.bc_loss_heads, backward().  Padding comes AFTER an episode's last step, so a padded
                                   step never feeds a real one.

Multi-rank: the expert set is replicated, every rank draws its own permutation, the gradient all-reduce is issued with
inv_n = 1 / (unmasked samples of the step x world).  It has never run on more than one rank.
Out of scope: soft targets / a KL distillation loss, several short episodes packed into one LSTM row, value
targets computed from expert returns (value_targets is taken if given), diagnostics for the cloning kernels.
"""
from __future__ import annotations

import numpy as np
import torch

from . import ops
from .dist_utils import allreduce_grad, allreduce_sum, collectives_on
from .gail import load_expert
from .policy import LSTMActorCritic, MLPActorCritic
from .range_guard import RangeGuard


def _read_expert(expert):
    """(states, actions, lengths or None) from the path of an .npz or a tuple of two / three arrays."""
    if isinstance(expert, (str, bytes)) or hasattr(expert, "__fspath__"):
        data = np.load(expert)
        return data["states"], data["actions"], (data["lengths"] if "lengths" in data.files else None)
    return expert[0], expert[1], (expert[2] if len(expert) > 2 else None)


def load_expert_sequences(expert, device):
    """(states f32 [E, Tmax, D], actions i32 [E, Tmax], lengths i64 [E] on the host) on `device` from the path of an .npz
    written by generate_expert_data(..., lengths=True) or a tuple (states [M, D], actions [M], lengths [E]): the flat pairs cut
    into episodes (episodes in order, steps in time order) and padded to the longest with zero states and action -1, the
    masked sample of the cloning kernels.  Raises without lengths, or when they do not sum to the number of pairs."""
    s, a, lengths = _read_expert(expert)
    if lengths is None:
        raise RuntimeError("expert sequences need the per-episode `lengths` (generate_expert_data(..., lengths=True))")
    s, a = load_expert((s, a), device)
    lengths = torch.as_tensor(np.asarray(lengths.cpu()) if torch.is_tensor(lengths) else np.asarray(lengths)).reshape(-1).to(torch.int64)
    M, E = s.shape[0], lengths.numel()
    if E == 0 or int(lengths.min()) < 1 or int(lengths.sum()) != M:
        raise RuntimeError(f"expert sequences: {E} episode lengths (each >= 1) summing to {int(lengths.sum()) if E else 0} for {M} pairs")
    T = int(lengths.max())
    ln = lengths.to(device)
    e = torch.repeat_interleave(torch.arange(E, device=device), ln)
    t = torch.arange(M, device=device) - torch.repeat_interleave(torch.cumsum(ln, 0) - ln, ln)
    states = torch.zeros(E, T, s.shape[1], dtype=torch.float32, device=device)
    actions = torch.full((E, T), -1, dtype=torch.int32, device=device)
    states[e, t] = s
    actions[e, t] = a
    return states, actions, lengths


class BCTrainer:
    """Clone `expert` into `policy` (an MLPActorCritic or an LSTMActorCritic).  expert: what gail.load_expert takes for an MLP,
    what load_expert_sequences takes for an LSTM.  epoch() = one optimiser step (gradient, all-reduce, uav_clip_adam on the
    trainer's own moments) per chunk of a fresh permutation -- `batch` rows of pairs for an MLP, `batch` whole episodes for an
    LSTM, the last chunk shorter as Tensor.split leaves it.  value_targets: f32, one per pair in the order of the pairs, or None;
    without them value_coef has nothing to act on.  metrics(): the last epoch's sums as means (one host read).
    Tests: forced_perms (index tensors consumed in order instead of drawn permutations), record (per-step sums, gradient norm,
    gradient and the parameters it was taken at in `log`).  Multi-rank: see the module docstring -- never run."""

    def __init__(self, policy, expert, *, batch=4096, lr=3e-4, value_coef=0.0, ent_beta=0.0, max_grad_norm=0.5, seed=0,
                 value_targets=None, rank=0, world_size=1):
        if isinstance(policy, LSTMActorCritic):
            self.kind = "lstm"
        elif isinstance(policy, MLPActorCritic):
            self.kind = "mlp"
        else:
            raise TypeError(f"BCTrainer: policy must be an MLPActorCritic or an LSTMActorCritic, got {type(policy).__name__}")
        if int(batch) < 1:
            raise ValueError(f"BCTrainer: batch={batch}")
        self.policy, self.device = policy, policy.device
        d = self.device
        self.batch, self.lr, self.max_grad_norm = int(batch), float(lr), float(max_grad_norm)
        self.value_coef, self.ent_beta = float(value_coef), float(ent_beta)
        self.seed, self.rank, self.world = int(seed), int(rank), int(world_size)
        self._coll = collectives_on()
        vt = None if value_targets is None else torch.as_tensor(value_targets).to(d, torch.float32).reshape(-1).contiguous()
        if self.kind == "lstm":
            self.obs, self.act, self.lengths = load_expert_sequences(expert, d)
            self.obs_dim = policy.obs_dim
            self.units = self.obs.shape[0]                       # what a permutation shuffles: episodes
            self._unit_count = ((self.act >= 0) & (self.act < 5)).sum(1)
            real = torch.arange(self.act.shape[1], device=d)[None, :] < self.lengths.to(d)[:, None]
            self._pad = ~real                                    # [E, Tmax]: the steps past each episode's end
            if vt is not None:
                if vt.numel() != int(self.lengths.sum()):
                    raise RuntimeError(f"value_targets: {vt.numel()} values for {int(self.lengths.sum())} pairs")
                pad = torch.zeros(self.act.shape, dtype=torch.float32, device=d)
                pad[real] = vt                                   # row-major over (episode, step) = the order of the pairs
                vt = pad
            self.fused_mlp = False
            self._work = {}                                      # episodes in a chunk -> the arrays its forward / backward write
        else:
            self.obs, self.act = load_expert(_read_expert(expert)[:2], d)
            self.obs_dim = policy.in_dim
            self.units = self.obs.shape[0]                       # rows
            self._unit_count = ((self.act >= 0) & (self.act < 5)).to(torch.int64)
            if vt is not None and vt.numel() != self.units:
                raise RuntimeError(f"value_targets: {vt.numel()} values for {self.units} pairs")
            # the fused kernel is the reference's network (6 + trend_k inputs, 256-128, 5 actions); False sends it down the layered path
            self.fused_mlp = 6 <= policy.in_dim <= 8 and (policy.h1, policy.h2, policy.n_act) == (256, 128, 5)
            self._stash = {}
        if self.obs.shape[-1] != self.obs_dim:
            raise RuntimeError(f"expert states have {self.obs.shape[-1]} features, the policy observes {self.obs_dim}")
        self.vtarget = vt
        self._all_valid = bool((self._unit_count == (self.act.shape[1] if self.kind == "lstm" else 1)).all())
        self.guard = RangeGuard(policy, self.kind, d, self.kind == "lstm" or self.fused_mlp)
        # the expert set never changes: measured once here against the fp16-split kernels' observation range, not every step
        self._obs_in_range = float(ops.absmax(self.obs.view(-1)).item()) < self.guard.limits[1]
        self._h0_probe = torch.zeros(1, dtype=torch.float32, device=d)
        self.exp_avg, self.exp_avg_sq = torch.zeros_like(policy.flat), torch.zeros_like(policy.flat)
        self.opt_step = 0
        self.gnorm = torch.zeros(1, dtype=torch.float32, device=d)
        self.bc_sums = torch.zeros(ops.BC_SUMS_N, dtype=torch.float64, device=d)
        self.epoch_sums = torch.zeros_like(self.bc_sums)
        self.forced_perms = None
        self.record = False
        self.log = []                # with record: (bc_sums, grad norm, all-reduced unclipped gradient, parameters it was taken at) per step
        self._perm_gen = None
        self.epochs_done = 0

    # ------------------------------------------------------------------------------------------
    def _next_perm(self):
        """One permutation of the expert set's rows (MLP) or episodes (LSTM), i64 on the device (VecPPOTrainer._next_perm's rule)."""
        L = self.units
        if self.forced_perms is not None:
            perm = torch.as_tensor(self.forced_perms.pop(0)).to(self.device).reshape(-1)
            if perm.numel() != L:
                raise ValueError(f"forced_perms: a permutation of {perm.numel()} for an expert set of {L}")
            return perm.to(torch.int64)
        if self._perm_gen is None:
            self._perm_gen = torch.Generator(device=self.device).manual_seed(self.seed * 1000003 + self.rank)
        return torch.randperm(L, generator=self._perm_gen, device=self.device)

    def _chunk_counts(self, chunks):
        """Unmasked samples of every chunk, as host ints; one host read per epoch, none when nothing is masked."""
        if self._all_valid:
            per = self.act.shape[1] if self.kind == "lstm" else 1
            return [c.numel() * per for c in chunks]
        return torch.stack([self._unit_count[c].sum() for c in chunks]).tolist()

    def _lstm_work(self, n):
        w = self._work.get(n)
        if w is None:
            T, H, f32 = self.obs.shape[1], self.policy.hidden, dict(dtype=torch.float32, device=self.device)
            w = {"work": {"dgates": ops.lstm_dgates(n, T, H, self.device), "heads": torch.empty(n, T, 6, **f32)},
                 "keep": torch.ones(n, T, **f32), "dheads": torch.empty(n * T, 6, **f32)}
            w["h0"], w["c0"] = self.policy.zero_state(n)
            for l in range(self.policy.num_layers):
                w["work"][f"stash{l}"] = torch.empty(n, T, 6 * H, **f32)
                w["work"][f"y{l}"] = torch.empty(n, T, H, **f32)
            self._work[n] = w
        return w

    def grad_of(self, chunk, count):
        """The cloning gradient of one chunk (i64 indices of rows / episodes; `count` its unmasked samples) into policy.grad,
        the step's sums into bc_sums."""
        pol = self.policy
        inv_n = 1.0 / float(max(int(count), 1) * self.world)
        if self.kind == "lstm":
            n = chunk.numel()
            w = self._lstm_work(n)
            # a padded step's input is zero whatever the resident set holds there: its heads are masked and it feeds no real
            # step, but a non-finite value would still reach the weight gradients as 0 x NaN through the gate derivatives
            obs = self.obs.index_select(0, chunk).masked_fill_(self._pad.index_select(0, chunk).unsqueeze(-1), 0.0)
            act = self.act.index_select(0, chunk).view(-1)
            vt = None if self.vtarget is None else self.vtarget.index_select(0, chunk).view(-1)
            heads = pol.heads(obs, w["keep"], w["h0"], w["c0"], w["work"])
            bias = pol.grad_views["head.bias"]                   # the loss kernel's column sums ARE this gradient
            ops.bc_loss_heads(heads.view(w["dheads"].shape), act, vt, inv_n, self.value_coef, self.ent_beta, self.bc_sums, w["dheads"], bias)
            return pol.backward(w["dheads"], w["work"], bias)
        if self.fused_mlp:
            return ops.mlp_bc_grad(pol.flat, self.obs, self.act, self.vtarget, inv_n, self.value_coef, self.ent_beta, self.bc_sums,
                                   pol.grad, trend_k=pol.in_dim - 6, rows=chunk.to(torch.int32))
        n = chunk.numel()
        if n not in self._stash:
            self._stash[n] = (torch.empty(n * (2 * pol.h1 + 2 * pol.h2 + 2), dtype=torch.float32, device=self.device),
                              torch.empty(n, pol.n_act + 1, dtype=torch.float32, device=self.device))
        stash, dheads = self._stash[n]
        heads = pol.heads(self.obs.index_select(0, chunk), stash=stash)
        vt = None if self.vtarget is None else self.vtarget.index_select(0, chunk)
        ops.bc_loss_heads(heads, self.act.index_select(0, chunk), vt, inv_n, self.value_coef, self.ent_beta, self.bc_sums, dheads)
        return pol.backward(dheads)

    def _optimiser_step(self, grad):
        allreduce_grad(grad)              # sum over ranks; inv_n already holds 1 / global count
        if self.record:
            kept = (grad.clone(), self.policy.flat.clone())
        self.opt_step += 1
        ops.clip_adam(self.policy.flat, grad, self.exp_avg, self.exp_avg_sq, self.opt_step, self.lr, max_norm=self.max_grad_norm,
                      gnorm_out=self.gnorm, pmax_out=self.guard.ranges[0:1])
        self.epoch_sums.add_(self.bc_sums)
        if self.record:
            self.log.append((self.bc_sums.clone(), self.gnorm.clone()) + kept)

    def epoch(self):
        """One pass over the expert set in shuffled chunks; returns the epoch's accumulated sums (device f64 [6])."""
        g = self.guard
        g.poll()
        self.epoch_sums.zero_()
        chunks = self._next_perm().split(self.batch)
        for chunk, count in zip(chunks, self._chunk_counts(chunks)):
            g.buffers_own = self._obs_in_range       # the resident expert set: measured at construction
            g.before_update(self.obs, self._h0_probe)
            self._optimiser_step(self.grad_of(chunk, count))
        g.after_update()
        self.epochs_done += 1
        return self.epoch_sums

    def metrics(self):
        """The last epoch as means over its unmasked samples: nll, value_loss (0.5 (V - R)^2, without value_coef), entropy,
        accuracy (argmax of the logits == the expert's action, with the parameters each step ran at) and samples.  One host
        read; raises on a NaN probability, on every rank together."""
        t = self.epoch_sums.clone()
        if self._coll:
            allreduce_sum(t)
        s = t.cpu().numpy()
        if s[3] > 0:
            raise RuntimeError("NaN in probs")
        n = max(float(s[5]), 1.0)
        return {"nll": float(s[0]) / n, "value_loss": float(s[1]) / n, "entropy": float(s[2]) / n, "accuracy": float(s[4]) / n,
                "samples": int(s[5])}
