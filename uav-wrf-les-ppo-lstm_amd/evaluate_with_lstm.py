"""evaluate_with_lstm.py -- greedy evaluation with an LSTM stop controller on the MI355X path.

Counterpart of the reference's PPOV2.0/evaluate_with_lstm.py (ThresholdController, :10-37; episode loop :67-101)
and PPOV2.1/evaluate_with_lstm.py (PeakAndStopPredictor :11-27; stop rule :69-77), vectorised: the reference's
1000 sequential episodes become N environments stepped together (one episode each), the greedy policy forward is
one uav_mlp_fwd / LSTM step per time step, and the stop predictors run through uav_lstm_fwd + uav_gemm_f32 +
uav_ln_relu.  Same class names, state_dict keys, metrics keys and decision rules as the reference; per-episode
Python scalars become device tensors of length N.  No CPU fallback: everything goes through uavppo.ops.

evaluate() also takes a policy object (the vectorised trainer's LSTMActorCritic / MLPActorCritic, or model.PPOActorCritic).
Where uav_greedy_episodes covers it (single-layer LSTM h = 64 / 128 or the reference's MLP, 6 observation features, the
fp16-split arithmetic, parameters inside that arithmetic's range) whole chunks of steps run in one launch each and the stop
controllers are replayed over the chunk's records, or (peak_stop_device, threshold_device) run as device scans over them.
Every other LSTM policy (stacked layers, h = 256, parameters beyond the fp16-split range, the other arithmetic modes) runs the
same chunk driver on the tail route: per env step the layers' step kernels and ONE uav_greedy_tail launch (heads, argmax, env
step, record), no host visit inside a chunk.  What is left (other MLPs, policy_probs functions) steps one launch sequence per
time step.  What the scripts share is in uavppo/greedy.py.
"""
from __future__ import annotations

import math
import os

import numpy as np
import torch

from config import EVALUATE_SIZE, SUCCESS_DISTANCE_THRESHOLD
from uavppo import ops
from uavppo.greedy import (GreedyRun, fused_refusal, policy_core, policy_route, stepwise_policy_probs,  # noqa: F401
                           tail_refusal)                                    # (fused_refusal, tail_refusal: tests, docs)
from uavppo.source_aniso import gather_truth
from uavppo.source_fit import SourceFit, is_aniso, variant_truth
from uavppo.source_fit import option as source_fit_option
from uavppo.source_stop import SourceStop
from uavppo.source_stop import option as source_stop_option

F32 = torch.float32


def _xavier(shape, gen):
    w = torch.empty(shape)
    torch.nn.init.xavier_uniform_(w, generator=gen)
    return w


class _DeviceLSTMStack:
    """nn.LSTM(input, hidden, num_layers, batch_first=True) in eval mode (no dropout), zero initial state."""

    def __init__(self, input_size, hidden_size, num_layers, device, gen, xavier):
        self.input_size, self.hidden_size, self.num_layers, self.device = input_size, hidden_size, num_layers, device
        self.p = {}
        k = 1.0 / math.sqrt(hidden_size)
        for l in range(num_layers):
            i = input_size if l == 0 else hidden_size
            for name, shape in ((f"weight_ih_l{l}", (4 * hidden_size, i)), (f"weight_hh_l{l}", (4 * hidden_size, hidden_size)),
                                (f"bias_ih_l{l}", (4 * hidden_size,)), (f"bias_hh_l{l}", (4 * hidden_size,))):
                if xavier:      # ConcentrationThresholdPredictor._init_weights, model.py:222-227
                    t = _xavier(shape, gen) if len(shape) > 1 else torch.zeros(shape)
                else:           # nn.LSTM default
                    t = (torch.rand(shape, generator=gen) * 2 - 1) * k
                self.p[name] = t.to(device=device, dtype=F32).contiguous()

    def last_output(self, x, lengths=None):
        """x [B, T, I] -> top layer output at the last valid step of every row [B, H]."""
        B, T, _ = x.shape
        H = self.hidden_size
        z = torch.zeros(B, H, dtype=F32, device=x.device)
        seq = x.contiguous()
        for l in range(self.num_layers):
            p = self.p
            seq, hn, cn, _ = ops.lstm_fwd(seq, None, z, z, p[f"weight_ih_l{l}"], p[f"weight_hh_l{l}"], p[f"bias_ih_l{l}"],
                                          p[f"bias_hh_l{l}"], want_stash=False)
        if lengths is None:
            return seq[:, T - 1].contiguous()
        idx = torch.as_tensor(lengths, device=x.device, dtype=torch.long) - 1          # pack_padded_sequence semantics
        return seq[torch.arange(B, device=x.device), idx].contiguous()


class ConcentrationThresholdPredictor:
    """PPOV2.0/model.py:203-240, inference: 3-layer LSTM(1 -> hidden) -> Linear(hidden, 64) -> LayerNorm(64) -> ReLU ->
    Linear(64, 1).  state_dict keys as the reference's nn.Module (lstm.*, fc.0.*, fc.1.*, fc.4.*)."""

    def __init__(self, input_size=1, hidden_size=128, device="cuda", seed=None):
        gen = torch.Generator().manual_seed(seed) if seed is not None else None
        self.device = torch.device(device)
        self.lstm = _DeviceLSTMStack(input_size, hidden_size, 3, self.device, gen, xavier=True)
        d = dict(device=self.device, dtype=F32)
        self.fc = {"fc.0.weight": _xavier((64, hidden_size), gen).to(**d), "fc.0.bias": torch.zeros(64, **d),
                   "fc.1.weight": torch.ones(64, **d), "fc.1.bias": torch.zeros(64, **d),
                   "fc.4.weight": _xavier((1, 64), gen).to(**d), "fc.4.bias": torch.zeros(1, **d)}

    def state_dict(self):
        sd = {f"lstm.{k}": v.clone() for k, v in self.lstm.p.items()}
        sd.update({k: v.clone() for k, v in self.fc.items()})
        return sd

    def load_state_dict(self, sd):
        for k in self.lstm.p:
            self.lstm.p[k].copy_(torch.as_tensor(np.asarray(sd[f"lstm.{k}"]), dtype=F32).reshape(self.lstm.p[k].shape))
        for k in self.fc:
            self.fc[k].copy_(torch.as_tensor(np.asarray(sd[k]), dtype=F32).reshape(self.fc[k].shape))

    def eval(self):
        return self

    def __call__(self, x, lengths=None):
        h = self.lstm.last_output(x, lengths)
        z = ops.gemm(h, self.fc["fc.0.weight"], trans_b=True, bias=self.fc["fc.0.bias"])
        a = ops.ln_relu(z, self.fc["fc.1.weight"], self.fc["fc.1.bias"])
        return ops.gemm(a, self.fc["fc.4.weight"], trans_b=True, bias=self.fc["fc.4.bias"]).reshape(-1)


class PeakAndStopPredictor:
    """PPOV2.1/evaluate_with_lstm.py:11-27: LSTM(1 -> hidden) -> h_n -> (Linear -> peak, Linear + Sigmoid -> stop_prob)."""

    def __init__(self, input_dim=1, hidden_dim=32, num_layers=1, device="cuda", seed=None):
        gen = torch.Generator().manual_seed(seed) if seed is not None else None
        self.device = torch.device(device)
        self.lstm = _DeviceLSTMStack(input_dim, hidden_dim, num_layers, self.device, gen, xavier=False)
        k = 1.0 / math.sqrt(hidden_dim)
        d = dict(device=self.device, dtype=F32)
        u = lambda shape: ((torch.rand(shape, generator=gen) * 2 - 1) * k).to(**d)
        # the two heads share one GEMM: rows = (peak, stop)
        self.heads_w, self.heads_b = torch.cat([u((1, hidden_dim)), u((1, hidden_dim))]).contiguous(), torch.cat([u((1,)), u((1,))])

    def state_dict(self):
        sd = {f"lstm.{k}": v.clone() for k, v in self.lstm.p.items()}
        sd.update({"fc_peak.weight": self.heads_w[0:1].clone(), "fc_peak.bias": self.heads_b[0:1].clone(),
                   "fc_stop.0.weight": self.heads_w[1:2].clone(), "fc_stop.0.bias": self.heads_b[1:2].clone()})
        return sd

    def load_state_dict(self, sd):
        for k in self.lstm.p:
            self.lstm.p[k].copy_(torch.as_tensor(np.asarray(sd[f"lstm.{k}"]), dtype=F32).reshape(self.lstm.p[k].shape))
        t = lambda k: torch.as_tensor(np.asarray(sd[k]), dtype=F32).to(self.device)
        self.heads_w.copy_(torch.cat([t("fc_peak.weight").reshape(1, -1), t("fc_stop.0.weight").reshape(1, -1)]))
        self.heads_b.copy_(torch.cat([t("fc_peak.bias").reshape(1), t("fc_stop.0.bias").reshape(1)]))

    def eval(self):
        return self

    def flat_params(self):
        """The predictor as uav_peak_stop_scan's one flat f32 buffer: the state_dict's tensors in its order (layer 0 of the LSTM)."""
        p = self.lstm.p
        return torch.cat([p["weight_ih_l0"].reshape(-1), p["weight_hh_l0"].reshape(-1), p["bias_ih_l0"], p["bias_hh_l0"],
                          self.heads_w[0], self.heads_b[0:1], self.heads_w[1], self.heads_b[1:2]]).contiguous()

    def __call__(self, x):
        if x.dim() == 2:
            x = x.unsqueeze(-1)
        h = self.lstm.last_output(x)
        out = ops.gemm(h, self.heads_w, trans_b=True, bias=self.heads_b)
        return out[:, 0], torch.sigmoid(out[:, 1])


class ThresholdController:
    """PPOV2.0/evaluate_with_lstm.py:10-37 for N environments at once.  `scaler` is anything with data_min_/data_max_
    (sklearn's MinMaxScaler) or a (min, max) pair.  The reference's per-episode `conc_buffer` and `trajectory[-window:]`
    are the same last-`window_size` concentrations, kept here as one [N, window] device tensor in time order."""

    def __init__(self, model, scaler, num_envs, window_size=EVALUATE_SIZE, device="cuda"):
        self.model, self.window_size, self.N = model, int(window_size), int(num_envs)
        self.device = torch.device(device)
        self.min_activate_steps = 2 * self.window_size
        lo, hi = ((float(scaler.data_min_[0]), float(scaler.data_max_[0])) if hasattr(scaler, "data_min_")
                  else (float(scaler[0]), float(scaler[1])))
        self.lo, self.scale = lo, (hi - lo) if hi != lo else 1.0
        self.reset()

    def reset(self):
        d = self.device
        self.window = torch.zeros(self.N, self.window_size, dtype=torch.float64, device=d)
        self.count = torch.zeros(self.N, dtype=torch.int64, device=d)
        self.current_threshold = torch.full((self.N,), float("nan"), dtype=torch.float64, device=d)   # NaN = None

    def push(self, current_conc):
        self.window = torch.roll(self.window, -1, dims=1)
        self.window[:, -1] = current_conc
        self.count += 1

    def update_threshold(self, active=None):
        """every 10th step of the loop (evaluate_with_lstm.py:87-88): envs whose trajectory is long enough"""
        ok = self.count >= max(self.window_size, self.min_activate_steps)
        if active is not None:
            ok &= active
        scaled = ((self.window - self.lo) / self.scale).to(F32).reshape(self.N, self.window_size, 1)
        pred = self.model(scaled, lengths=None).to(torch.float64) * 0.95
        self.current_threshold = torch.where(ok, pred, self.current_threshold)

    def should_stop(self, current_conc, step_count):
        w = self.window_size
        n = torch.clamp(self.count, max=w).to(torch.float64)
        valid = (torch.arange(w, device=self.device)[None, :] >= (w - torch.clamp(self.count, max=w))[:, None])
        mean = (self.window * valid).sum(1) / torch.clamp(n, min=1.0)
        has = ~torch.isnan(self.current_threshold)
        thr = torch.nan_to_num(self.current_threshold, nan=float("inf"))
        return (step_count >= self.min_activate_steps) & has & ((current_conc >= thr) | (mean >= thr))


def peak_stop_refusal(peak_stop, window):
    """Why uav_peak_stop_scan cannot run `peak_stop` over windows of `window` steps (None when it can)."""
    l = peak_stop.lstm
    if l.hidden_size != 32 or l.num_layers != 1 or l.input_size != 1:
        return (f"the predictor has hidden {l.hidden_size}, {l.num_layers} layer(s), input_dim {l.input_size}; uav_peak_stop_scan "
                f"covers hidden 32, one layer, input_dim 1")
    if not 1 <= int(window) <= 32:
        return f"window_size_v21 = {window}; uav_peak_stop_scan takes windows of 1 .. 32 steps"
    return None


class _DevicePeakStop:
    """The PPOV2.1 rule on uav_peak_stop_scan: the predictor's flat parameters and the envs' last window - 1 inputs."""

    def __init__(self, peak_stop, window, N, device):
        why = peak_stop_refusal(peak_stop, window)
        if why is not None:
            raise RuntimeError(f"evaluate(peak_stop_device=True): {why}")
        self.params, self.hidden, self.window = peak_stop.flat_params(), peak_stop.lstm.hidden_size, int(window)
        self.hist = torch.zeros(N, self.window - 1, dtype=F32, device=device)
        self.cnt = torch.zeros(N, dtype=torch.int32, device=device)

    def scan(self, series, active=None):
        """series f32 [N, k] (any strides) -> (first_hit i32 [N], peak f32 [N, k], prob f32 [N, k])"""
        return ops.peak_stop_scan(self.params, self.hidden, self.window, series, self.hist, self.cnt, active=active, prob_min=0.8)


class _DeviceThreshold:
    """The PPOV2.0 rule on uav_threshold_windows / uav_threshold_rule around one batched call of the controller's predictor: the
    envs' last window - 1 inputs, their step counts and their thresholds (f64, NaN = none yet)."""
    EVERY = 10          # the episode loop's `step_count % 10 == 0` (PPOV2.0/evaluate_with_lstm.py:87)

    def __init__(self, controller, N, device):
        self.model, self.lo, self.scale = controller.model, float(controller.lo), float(controller.scale)
        self.window, self.min_steps = int(controller.window_size), int(controller.min_activate_steps)
        if not 1 <= self.window <= 32:
            raise RuntimeError(f"evaluate(threshold_device=True): window_size = {self.window}; uav_threshold_rule takes windows of "
                               f"1 .. 32 steps")
        self.N = int(N)
        self.hist = torch.zeros(N, self.window - 1, dtype=F32, device=device)
        self.cnt = torch.zeros(N, dtype=torch.int32, device=device)
        self.thr = torch.full((N,), float("nan"), dtype=torch.float64, device=device)
        self._no_pred = {}

    def has_update(self, t0, k):
        """whether an env that enters with t0 steps behind it meets an update step within the next k"""
        first = max(t0 + 1, self.window, self.min_steps)
        return -(-first // self.EVERY) * self.EVERY <= t0 + k

    def scan(self, series, active=None, t0=None, want_steps=False):
        """series f32 [N, k] (any strides) -> (first_hit i32 [N], stop u8 [N, k] or None, thr f64 [N, k] or None).  t0: the steps
        every active env has behind it, where the caller knows it: a call that can hold no update step skips the predictor."""
        k = int(series.shape[1])
        S = ops.threshold_slots(k, self.EVERY)
        kw = dict(active=active, window=self.window, every=self.EVERY, min_steps=self.min_steps)
        if t0 is None or self.has_update(t0, k):
            x = ops.threshold_windows(series, self.hist, self.cnt, lo=self.lo, scale=self.scale, **kw)
            pred = self.model(x.reshape(self.N * S, self.window, 1)).to(F32).reshape(self.N, S).contiguous()
        else:           # no slot is read
            if S not in self._no_pred:
                self._no_pred[S] = torch.zeros(self.N, S, dtype=F32, device=series.device)
            pred = self._no_pred[S]
        return ops.threshold_rule(series, self.hist, self.cnt, pred, self.thr, factor=0.95, want_steps=want_steps, **kw)


class _StopRules:
    """The stop rules of one evaluate() call -- the PPOV2.0 ThresholdController and the PPOV2.1 PeakAndStopPredictor, each on the host
    or on the device -- behind one loop body, step().  Resets the controller.  `replay` is true while some rule given is NOT on the
    device: the fused path then walks a chunk's records through step(); otherwise first_hits() of the chunk's scan is all it needs."""

    def __init__(self, controller, peak_stop, window_size_v21, N, device, peak_stop_device, threshold_device):
        self.controller, self.peak_stop, self.window, self.N, self.device = controller, peak_stop, window_size_v21, N, device
        if controller is not None:
            controller.reset()
        self.peak_pred = torch.full((N,), float("nan"), dtype=torch.float64, device=device)
        self.traj = torch.zeros(N, window_size_v21, dtype=torch.float64, device=device) if peak_stop is not None else None
        self.dps = _DevicePeakStop(peak_stop, window_size_v21, N, device) if peak_stop_device and peak_stop is not None else None
        self.dth = _DeviceThreshold(controller, N, device) if threshold_device and controller is not None else None
        self.any = controller is not None or peak_stop is not None
        self.replay = (controller is not None and self.dth is None) or (peak_stop is not None and self.dps is None)
        self.peak_hit = self.thr_hit = self.peak_c = None

    def scan(self, series, active, t0, want_steps):
        """The device rules over series f32 [N, k] (any strides), the concentrations of steps t0 + 1 .. t0 + k; their outputs are kept
        for step() and first_hits().  active bool [N]: every active env has t0 steps behind it.  want_steps: step() will be called."""
        if self.dps is None and self.dth is None:
            return
        active = active.to(torch.uint8)
        if self.dps is not None:
            self.peak_hit, self.peak_c, self.prob_c = self.dps.scan(series, active)
        if self.dth is not None:
            self.thr_hit, self.thr_stop, _ = self.dth.scan(series, active, t0, want_steps=want_steps)

    def step(self, i, t, conc, active):
        """The loop body (PPOV2.0/evaluate_with_lstm.py:84-92, PPOV2.1/evaluate_with_lstm.py:69-77) at step t, column i of the last
        scan: conc f32 [N], the concentration record -> stop_now bool [N].  Host rules advance by this step."""
        controller, traj = self.controller, self.traj
        cur = conc.to(torch.float64) * 100.0                   # conc_field at the agent
        stop_now = torch.zeros(self.N, dtype=torch.bool, device=self.device)
        if self.dth is not None:
            stop_now |= self.thr_stop[:, i] != 0
        elif controller is not None:
            controller.push(cur)
            if t % 10 == 0:
                controller.update_threshold(active)
            stop_now |= controller.should_stop(cur, t)
        peak = prob = None
        if self.dps is not None:                               # NaN (no hit) until the env's window is full
            peak, prob = self.peak_c[:, i], self.prob_c[:, i]
        elif self.peak_stop is not None:
            self.traj = traj = torch.roll(traj, -1, dims=1)
            traj[:, -1] = cur
            if t >= self.window:
                peak, prob = self.peak_stop((traj / 100.0).to(F32))
        if prob is not None:
            hit = prob > 0.8
            self.peak_pred = torch.where(hit & active, peak.to(torch.float64), self.peak_pred)   # recorded whenever the LSTM stopped it (:85-87)
            stop_now |= hit
        return stop_now

    def first_hits(self, k):
        """(at_peak, at_thr) of the last scan over k steps: per env the chunk step of each device rule's first hit as i64 [N], k where
        it has none; the plain int k for a rule that is not there."""
        return tuple(k if hit is None else torch.where(hit >= 0, hit.to(torch.int64), k) for hit in (self.peak_hit, self.thr_hit))

    def finish(self, out):
        if self.dth is not None:
            self.controller.current_threshold = self.dth.thr
        if self.peak_stop is not None:
            out["peak_pred"] = self.peak_pred.cpu().numpy()
        return out


class _Episodes:
    """Per env of an evaluate() call: whether its episode still runs, and the step, the position and the cause of its end.  Torch
    tensor operations only."""

    def __init__(self, N, device):
        self.active = torch.ones(N, dtype=torch.bool, device=device)
        self.steps = torch.zeros(N, dtype=torch.int64, device=device)
        self.stopped = torch.zeros(N, dtype=torch.bool, device=device)
        self.final_pos = torch.zeros(N, 2, dtype=torch.float64, device=device)
        self.rows = torch.arange(N, device=device)
        self.cols = self.rows[:0]

    def end(self, ended, t, by_rule, pos_end):
        """The episodes `ended` (bool [N], all of them active) end with step t (an int, or i64 [N]) at pos_end f64 [N, 2]; by_rule
        bool [N] or None: a stop rule fired on that step (the reference sets the flag whenever the controller fires on the last step)."""
        self.steps = torch.where(ended, t, self.steps)
        if by_rule is not None:
            self.stopped |= ended & by_rule
        self.final_pos = torch.where(ended[:, None], pos_end, self.final_pos)
        self.active ^= ended                      # `ended` lies within `active`: clears exactly those

    def end_chunk(self, t0, k, done_c, obs, pos, at_peak, at_thr, peak_c=None, peak_pred=None):
        """end() for the k steps t0 + 1 .. t0 + k at once: an episode ends at min(first done record, each rule's first hit).  done_c
        bool [N, k], obs [N, k, D], pos [N, k, 2]: the chunk's records; at_peak, at_thr: _StopRules.first_hits(k); peak_c f32 [N, k] or
        None: the peak-stop rule's peaks.  Returns peak_pred with the peak of every episode that rule ended."""
        rows = self.rows
        if self.cols.numel() != k:
            self.cols = torch.arange(k, device=rows.device)
        at_done = torch.where(done_c, self.cols, k).amin(1)                           # k = none in this chunk
        hits = [a for a in (at_peak, at_thr) if torch.is_tensor(a)]
        at_hit = torch.minimum(*hits) if len(hits) == 2 else hits[0] if hits else None
        first = at_done if at_hit is None else torch.minimum(at_done, at_hit)
        ended = self.active & (first < k)
        if peak_c is not None:
            by_peak = ended & (at_peak <= first)      # the peak-stop rule fired on the episode's last step (alone or beside the others)
        first = first.clamp(max=k - 1)
        pos_end = obs[rows, first, :2].to(torch.float64) * 500.0                      # the record is the terminal obs where done
        if at_hit is not None:
            pos_end = torch.where((ended & (at_done <= at_hit))[:, None], pos_end, pos[rows, first].to(torch.float64))
        if peak_c is not None:
            peak_pred = torch.where(by_peak, peak_c[rows, first].to(torch.float64), peak_pred)
        self.end(ended, first + (t0 + 1), None if at_hit is None else at_hit <= at_done, pos_end)
        return peak_pred

    def metrics(self, src, limit, last_pos, success_distance):
        """The reference's metrics dict against the sources src f64 [N, 2].  Episodes still active were cut off by `max_steps`:
        they took `limit` steps and stand at last_pos [N, 2]."""
        final_pos = torch.where(self.active[:, None], last_pos.to(torch.float64), self.final_pos)
        steps = torch.where(self.active, limit, self.steps)
        deviation = torch.linalg.norm(final_pos - src, dim=1)
        return {"deviations": deviation.cpu().numpy(), "steps": steps.cpu().numpy(),
                "success": (deviation <= success_distance).cpu().numpy(), "stopped_early": self.stopped.cpu().numpy()}


def _begin(env, controller, peak_stop, window_size_v21, peak_stop_device, threshold_device, max_steps):
    """Resets the env, then the controller -> (source positions, _Episodes, _StopRules, step limit)"""
    env.reset()
    _, src, _, _ = env.peek()
    rules = _StopRules(controller, peak_stop, window_size_v21, env.num_envs, env.device, peak_stop_device, threshold_device)
    return src.clone(), _Episodes(env.num_envs, env.device), rules, max_steps or env.max_steps


@torch.no_grad()
def evaluate(policy_probs, env, controller=None, peak_stop=None, window_size_v21=20, noise=None, max_steps=None,
             success_distance=SUCCESS_DISTANCE_THRESHOLD, fused=None, chunk=None, peak_stop_device=False, threshold_device=False,
             tail=None, source_fit=None, source_stop=None, bank_truth=None):
    """One greedy episode per environment of `env` (a uavppo VecMethaneEnv), all N together.

    policy_probs(obs [N, obs_dim]) -> probs or logits [N, 5] (argmax is taken), or a policy object: LSTMActorCritic,
    MLPActorCritic or model.PPOActorCritic (the LSTM starts every episode from zero state);
    controller: ThresholdController (PPOV2.0 rule) or None; peak_stop: PeakAndStopPredictor (PPOV2.1 rule) or None;
    noise: optional f64 [steps, N, 2] (parity tests).  Returns the reference's metrics dict (deviations, steps, success,
    stopped_early [, peak_pred]) as numpy arrays of length N.
    fused (policy objects): None = uav_greedy_episodes where it covers the policy (fused_refusal), else step-wise (parameters
    beyond the fp16-split range then run in bf16x6); True = the fused kernel or a RuntimeError naming why not; False =
    step-wise.  tail (policy objects): None = where the fused kernel refuses the policy and the tail route covers it
    (tail_refusal: any LSTMActorCritic of 5 actions, hidden a multiple of 4 up to 256), the tail route -- the LSTM layers' step
    kernels and one uav_greedy_tail per env step under the fused path's chunk driver, the same metric arrays as the step-wise
    loop bit for bit; True = the tail route or a RuntimeError naming why not; False = never.  fused=False alone still means
    step-wise, fused=True the fused kernel or an error.  chunk: steps per fused launch, or per host visit of the tail route
    (default: 250, or 50 with a stop controller, whose rules are replayed over each chunk's records).  A NaN logit of a policy
    object raises RuntimeError("NaN in probs").  A policy_probs function takes none of fused=True, tail=True and chunk.
    peak_stop_device=True: the PPOV2.1 rule runs on uav_peak_stop_scan -- one scan over all sliding windows of a fused chunk's
    records, or one scan of steps = 1 per env step on the step-wise path.  Same decisions and metrics as the default, which
    evaluates the predictor through uav_lstm_fwd + uav_gemm_f32 (peak_pred agrees to the f32 kernels' rounding); a predictor the
    kernel does not cover (peak_stop_refusal) raises RuntimeError.
    threshold_device=True: the PPOV2.0 rule runs on the device -- per fused chunk uav_threshold_windows, ONE batched call of the
    controller's predictor over the chunk's windows, and uav_threshold_rule, or the rule kernel with steps = 1 per env step on the
    step-wise path (windows and predictor on update steps only).  Same decisions and metrics as the default (the window mean is
    summed in np.mean's order, as the reference's, where the host replay uses torch's sum).  On return controller.current_threshold
    holds the device's thresholds (f64 [N], NaN = None; an env that ended inside a fused chunk has that chunk's last).
    source_fit: None (off), True or a dict of uavppo.source_fit.check_source_fit's keywords: where the episode's measurements say
    the source is -- one uav_source_moments per chunk of records, uav_source_solve and uav_source_summary after the last.  The
    metrics gain source_estimate f64 [N, 2], source_sigma, source_peak, source_strength, source_status u8 (ops.SRC_STATUS_NAMES),
    source_error (NaN unless fitted) and source_max_sample f64 [N, 3] (x, y, b of the largest sample); nothing else changes.
    Fused and tail routes only, and without controller / peak_stop (their hits are not in the records' flags): else ValueError.
    source_stop: None (off), True or a dict of uavppo.source_stop.check_source_stop's keywords: the estimator as the stop rule --
    per chunk the greedy chunk, uav_source_stop_scan (which writes its hits into the records' flags), then uav_source_moments.  An
    episode ends where the fit has settled and the UAV stands within `near` of it: stopped_early is true for those, steps,
    deviations and success refer to where the UAV stopped, the source_* metrics are the estimator on the records up to the stop
    (source_stop implies source_fit; its keywords are the source_fit= dict or the defaults), and source_stop_step i64 [N] is the
    step the rule fired at, 0 where it did not.  The env's own success radius still ends episodes: make it small where the rule is
    to do the stopping.  Refused as source_fit is: with controller / peak_stop, and on the step-wise route.
    source_fit={"model": "aniso"}: the six-term fit of a plume stretched along an axis (uavppo/source_aniso.py; the uav_source_*6
    kernels).  source_sigma is then the major width and the metrics gain source_sigma_minor and source_theta.  bank_truth: f64
    [F, 4] = {sigma_major, sigma_minor, theta, peak} per field of the env's bank (field_bank.load_with_truth) or None: what the
    summary scores the widths, the angle, the peak and the strength against, gathered per env on the device by env_core.h's field
    rule.  Not together with source_stop (its scan is four-term): ValueError."""
    fit_cfg, stop_cfg = source_fit_option(source_fit), source_stop_option(source_stop)
    if is_aniso(fit_cfg) and stop_cfg is not None:
        raise ValueError("evaluate(source_stop=...): not with source_fit model \"aniso\": the stop scan solves the four-term system "
                         "per record; a six-term scan does not exist")
    if bank_truth is not None and not is_aniso(fit_cfg):
        raise ValueError("evaluate(bank_truth=...): only the six-term estimator (source_fit={\"model\": \"aniso\"}) scores against it")
    if stop_cfg is not None:
        if controller is not None or peak_stop is not None:
            raise ValueError("evaluate(source_stop=...): not together with controller / peak_stop: their hits are not in the records' "
                             "flags, so the estimator could not know where those episodes ended")
        fit_cfg = fit_cfg if fit_cfg is not None else source_fit_option(True)
    if fit_cfg is not None and (controller is not None or peak_stop is not None):
        raise ValueError("evaluate(source_fit=...): not together with controller / peak_stop: their hits are not in the records' "
                         "flags, so the estimator could not know where those episodes ended")
    pc, nan = policy_core(policy_probs), None
    if pc is None and fused:
        raise RuntimeError("evaluate(fused=True): a policy_probs function has no fused kernel; pass the policy object")
    if pc is None and tail:
        raise RuntimeError("evaluate(tail=True): a policy_probs function has no tail route; pass the policy object")
    if pc is None and chunk is not None:
        raise ValueError("evaluate(chunk=...): chunks belong to the fused path of a policy object")
    if pc is not None:
        kind, core = pc
        route = policy_route(policy_probs, env, fused, tail, "evaluate")
        if route != "stepwise":
            return _evaluate_fused(kind, core, env, controller, peak_stop, window_size_v21, noise, max_steps, success_distance,
                                   chunk, peak_stop_device, threshold_device, tail=route == "tail", fit_cfg=fit_cfg, stop_cfg=stop_cfg,
                                   bank_truth=bank_truth)
        policy_probs, nan = stepwise_policy_probs(kind, core, env)
    if stop_cfg is not None:
        raise ValueError("evaluate(source_stop=...): the rule reads the records of the fused and tail routes; the step-wise route "
                         "keeps none")
    if fit_cfg is not None:
        raise ValueError("evaluate(source_fit=...): the estimator reads the records of the fused and tail routes; the step-wise "
                         "route keeps none")
    src, ep, rules, limit = _begin(env, controller, peak_stop, window_size_v21, peak_stop_device, threshold_device, max_steps)
    N, obs = env.num_envs, env.obs
    for t in range(1, limit + 1):
        act = torch.argmax(policy_probs(obs), dim=1).to(torch.int32)
        obs, _, done, _ = env.step(act, None if noise is None else noise[t - 1])
        done_b = done > 0.5
        conc = torch.where(done_b, env.term_obs[:, 2], obs[:, 2])
        pos_now, _, _, _ = env.peek()
        pos_end = torch.where(done_b[:, None], env.term_obs[:, :2].to(torch.float64) * 500.0, pos_now.to(torch.float64))
        # the device rules, steps = 1.  Both get `active`; the peak-stop scan once ran over all envs, which changes nothing that is read:
        # an inactive env never becomes active again, its hit is masked by `ended = active & ...`, peak_pred is gated by `hit & active`
        rules.scan(conc.reshape(N, 1), ep.active, t - 1, True)
        stop_now = rules.step(0, t, conc, ep.active)
        ep.end(ep.active & (done_b | stop_now), t, stop_now, pos_end)
        if t % 16 == 0 and not bool(ep.active.any()):
            break
    if nan is not None and int(nan.item()) > 0:
        raise RuntimeError("NaN in probs")                                       # model.py:47-49
    return rules.finish(ep.metrics(src, limit, pos_now, success_distance))


def _evaluate_fused(kind, core, env, controller, peak_stop, window_size_v21, noise, max_steps, success_distance, chunk,
                    peak_stop_device=False, threshold_device=False, tail=False, fit_cfg=None, stop_cfg=None, bank_truth=None):
    """evaluate() on uav_greedy_episodes: `chunk` steps per launch (tail: on GreedyRun's tail backend, `chunk` steps per host visit); the metrics (and the stop controllers) are computed from
    the records by the step-wise loop's own _StopRules.step / _Episodes.end, so the same actions give the same arrays bit for
    bit.  An env the kernel has ended stays frozen (no auto-reset); an env a rule stopped goes into the next chunk inactive.
    Only while some rule given is NOT on the device (rules.replay) are the records walked step by step, the device rules' per-step
    flags among them; otherwise -- every rule on the device, or none given -- a chunk is one _Episodes.end_chunk.  stop_cfg: the
    estimator's stop rule scans each chunk before anything else reads it; its first hits go into end_chunk as a device rule's do."""
    src, ep, rules, limit = _begin(env, controller, peak_stop, window_size_v21, peak_stop_device, threshold_device, max_steps)
    run = GreedyRun(kind, core, env, tail=tail)
    aniso = is_aniso(fit_cfg)
    fit = SourceFit(env.num_envs, env.device, **fit_cfg) if fit_cfg is not None else None
    truth = gather_truth(bank_truth, env) if aniso else None        # where src was taken: after the reset, before the first step
    stop = SourceStop(env.num_envs, env.device, fit_cfg=fit_cfg, **stop_cfg) if stop_cfg is not None else None
    chunk = int(chunk or (50 if rules.any else 250))
    t0 = 0
    while t0 < limit:
        k = min(chunk, limit - t0)
        recs = run.chunk(t0, k, noise)
        ended = (~ep.active).to(torch.uint8) if fit is not None else None     # before this chunk's ends are taken
        at_stop = k
        if stop is not None:                         # marks its hits in the flags and clears the kernel's `active` there
            hit = stop.scan(recs, t0, ended, run.active)
            at_stop = torch.where(hit >= 0, hit.to(torch.int64), k)
        if fit is not None:
            fit.chunk(recs, ended)
        done_c = (recs["flags"] & 1) != 0
        conc = recs["obs"][:, :, 2]                  # the record is the terminal obs where done
        rules.scan(conc, ep.active, t0, rules.replay)   # `active` is the kernel's as the launch found it (the kernel clears it at `done`)
        if rules.replay:
            for i in range(k):                       # evaluate()'s loop body, step t = t0 + i + 1, on the records
                done_b = done_c[:, i]
                pos_end = torch.where(done_b[:, None], recs["obs"][:, i, :2].to(torch.float64) * 500.0, recs["pos"][:, i].to(torch.float64))
                stop_now = rules.step(i, t0 + i + 1, conc[:, i], ep.active)
                ep.end(ep.active & (done_b | stop_now), t0 + i + 1, stop_now, pos_end)
        else:
            at_peak, at_thr = rules.first_hits(k)
            rules.peak_pred = ep.end_chunk(t0, k, done_c, recs["obs"], recs["pos"], at_peak, at_thr if stop is None else at_stop,
                                           rules.peak_c, rules.peak_pred)
        if rules.any:
            run.retire(ep.active)
        last_pos = recs["pos"][:, k - 1]             # episodes cut off by `max_steps` are still active, so stepped through the last record
        t0 += k
        if not bool(ep.active.any()):
            break
    run.raise_on_nan()
    out = rules.finish(ep.metrics(src, limit, last_pos, success_distance))
    if fit is not None:                              # the four-term model's truth is the variant's, the six-term model's per env
        sigma_true, peak_true = variant_truth(env.variant) if env.bank is None else (float("nan"), float("nan"))
        fit.finish(src.to(torch.float64).contiguous(), sigma_true, peak_true, truth=truth)
        out.update(fit.metrics())
    if stop is not None:
        out["source_stop_step"] = stop.stop_steps().cpu().numpy()
    return out


def load_lstm_policy(path, device="cuda"):
    """An LSTMActorCritic from a vectorised-trainer checkpoint (train_ppo2.0.py's _save: lstm.*, actor.*, critic.*), its
    obs_dim / hidden / layers / actions read off the tensor shapes."""
    from uavppo.policy import LSTMActorCritic
    sd = torch.load(path, map_location="cpu")
    layers = sum(1 for k in sd if k.startswith("lstm.weight_ih_l"))
    w0 = sd["lstm.weight_ih_l0"]
    pol = LSTMActorCritic(obs_dim=int(w0.shape[1]), hidden=int(w0.shape[0]) // 4, num_layers=layers,
                          n_act=int(sd["actor.weight"].shape[0]), device=device)
    pol.load_state_dict(sd)
    return pol


def main(num_envs=1000, model_dir="model", device="cuda", policy="mlp", threshold_device=False, source_stop=False):
    """The reference's main() (evaluate_with_lstm.py:39-134) with its 1000 episodes run as 1000 parallel environments.
    policy="mlp": the reference's PPOActorCritic; "lstm": the vectorised trainer's LSTM actor-critic (same file name).
    threshold_device (--device-rule): the ThresholdController's rule on the device (evaluate(threshold_device=True)).
    source_stop (--source-stop, with --lstm): no ThresholdController -- the source estimator itself stops the episodes
    (evaluate(source_stop=True)) in an env of success radius 2; prints where it stopped and how well it located the source."""
    from model import PPOActorCritic
    from uavppo.vec_env import VecMethaneEnv
    if policy not in ("mlp", "lstm"):
        raise ValueError(f"main: policy must be 'mlp' or 'lstm', got {policy!r}")
    if source_stop and policy != "lstm":
        raise ValueError("main: --source-stop reads the records of a policy object; use it with --lstm")
    try:
        path = os.path.join(model_dir, "ppo_successful_models.pth")
        if policy == "lstm":
            ppo_model = load_lstm_policy(path, device)
        else:
            sd = torch.load(path, map_location="cpu")
            ppo_model = PPOActorCritic(int(sd["feature.0.weight"].shape[1]), 5, device=device)     # 6, or 6 + TREND_K
            ppo_model.load_state_dict(sd)
        if not source_stop:                                      # the estimator's rule needs no predictor and no scaler
            lstm_model = ConcentrationThresholdPredictor(device=device)
            lstm_model.load_state_dict(torch.load(os.path.join(model_dir, "lstm_threshold_predictor.pth"), map_location="cpu"))
            scaler_params = np.load(os.path.join(model_dir, "scaler_params.npy"))
    except FileNotFoundError as e:
        print(f"model files missing: {e}")
        return None
    trend_k = (ppo_model.obs_dim if policy == "lstm" else ppo_model.core.in_dim) - 6
    env = VecMethaneEnv(num_envs, "v2.0", device, trend_k=trend_k)
    if not source_stop:
        controller = ThresholdController(lstm_model, (scaler_params.min(), scaler_params.max()), num_envs, device=device)
    if source_stop:
        env.current_radius = 2.0
        metrics = evaluate(ppo_model, env, source_stop=True)
        fit = metrics["source_status"] == 0
        print(f"stopped by the estimator: {metrics['stopped_early'].mean() * 100:.1f}%  fitted: {fit.mean() * 100:.1f}%  "
              f"median estimate error: {np.median(metrics['source_error'][fit]) if fit.any() else float('nan'):.2f} px")
    elif policy == "lstm":
        metrics = evaluate(ppo_model, env, controller, threshold_device=threshold_device)
    else:                                                                                  # argmax of logits == argmax of probs
        metrics = evaluate(lambda o: ppo_model.core.heads(o)[:, :5], env, controller, threshold_device=threshold_device)
    ok = metrics["success"]
    print("===== validation =====")
    print(f"mean deviation: {metrics['deviations'].mean():.2f} +- {metrics['deviations'].std():.2f} px")
    if ok.any():
        print(f"mean deviation of successes: {metrics['deviations'][ok].mean():.2f} +- {metrics['deviations'][ok].std():.2f} px")
    print(f"success rate: {ok.mean() * 100:.1f}%  early-stop rate: {metrics['stopped_early'].mean() * 100:.1f}%  "
          f"mean steps: {metrics['steps'].mean():.1f}")
    os.makedirs("results", exist_ok=True)
    np.savez("results/validation_metrics.npz", **metrics)
    return metrics


if __name__ == "__main__":
    import sys
    main(policy="lstm" if "--lstm" in sys.argv[1:] else "mlp", threshold_device="--device-rule" in sys.argv[1:],
         source_stop="--source-stop" in sys.argv[1:])
