"""Step-size and entropy-weight schedules of VecPPOTrainer: lr_schedule = "constant" | "linear" | "adaptive", and
ent_beta_final beside any of them.

Definitions (f64):
  linear    value(k) = start + (final - start) * min(k, K) / K,  k = trainer.iteration (0-based), K = schedule_iterations; the
            value is cast to float where a kernel takes it, as hp["lr"] and hp["ent_beta"] are
  adaptive  after every update, from the eight all-reduced diagnostic sums S of the LAST epoch that ran (ops.PPO_DIAG_NAMES):
            n = S[7], kl = S[1] / n (the k3 estimate that target_kl and diagnostics()["approx_kl"] use), and
              n > 0 is false, or kl is a NaN   the rate stays; skipped += 1
              kl > 2 * desired_kl              lr = max(lr / factor, lr_min); lowered += 1      (+inf lowers)
              kl < desired_kl / 2              lr = min(lr * factor, lr_max); raised += 1
              otherwise                        held += 1                                        (both edges hold)
            The new rate is the next update's; all optimiser steps of one update share one rate.

linear_value / adapt_rule state the definitions in numpy: what the kernels (csrc/lr_control.hip) and the trainer are tested
against, and what a log reader replays a run with.  LrController owns the device state of the adaptive rule and the f32 rate
uav_clip_adam_dlr reads; no host read on the path.
"""
from __future__ import annotations

import numpy as np
import torch

from . import ops

STATE_N = ops.LR_STATE_N             # lr, last_kl, raised, lowered, held, skipped
SCHEDULES = ("constant", "linear", "adaptive")
STATE_FILE = "lr_state.npz"

_NUM = (int, float, np.integer, np.floating)


def _number(v):
    return isinstance(v, _NUM) and not isinstance(v, bool)


def _finite(v, lowest=None):
    """v is a finite number (greater than `lowest` where one is given)."""
    return _number(v) and abs(float(v)) < float("inf") and (lowest is None or float(v) > lowest)


def check_lr_control(lr_schedule="constant", lr=3e-5, lr_final=None, ent_beta_final=None, schedule_iterations=None,
                     desired_kl=None, lr_factor=1.5, lr_min=1e-6, lr_max=1e-2, optimiser_steps=None):
    """VecPPOTrainer's schedule keywords, refused with the reason (ValueError) where they contradict each other; returns them as
    a dict of plain floats / ints / None.  optimiser_steps: the optimiser steps of one update (epochs * steps per epoch).  Pure
    host arithmetic: VecPPOTrainer calls it before it allocates anything.  The bounds lr_min, lr_max and lr_factor are checked
    under every schedule; that the starting lr lies inside them only where they act, under "adaptive"."""
    if lr_schedule not in SCHEDULES:
        raise ValueError(f"lr_schedule {lr_schedule!r}: one of {', '.join(repr(s) for s in SCHEDULES)}")
    if lr_schedule == "linear" or ent_beta_final is not None:
        K = schedule_iterations
        if isinstance(K, bool) or not isinstance(K, (int, np.integer)) or K < 1:
            raise ValueError(f"schedule_iterations={K!r}: lr_schedule='linear' and ent_beta_final interpolate over a positive "
                             "number of iterations")
    if lr_schedule == "linear" and not (_finite(lr_final) and float(lr_final) >= 0.0):
        raise ValueError(f"lr_final={lr_final!r}: lr_schedule='linear' needs the rate it ends at, a finite number >= 0")
    if lr_schedule != "linear" and lr_final is not None:
        raise ValueError(f"lr_final={lr_final!r} without lr_schedule='linear' would be ignored")
    if ent_beta_final is not None and not (_finite(ent_beta_final) and float(ent_beta_final) >= 0.0):
        raise ValueError(f"ent_beta_final={ent_beta_final!r}: a finite number >= 0, or None")
    if not (_number(lr_factor) and float(lr_factor) > 1.0):
        raise ValueError(f"lr_factor={lr_factor!r}: a number greater than 1")
    if not (_number(lr_min) and float(lr_min) > 0.0):
        raise ValueError(f"lr_min={lr_min!r}: a positive number")
    if not (_number(lr_max) and float(lr_min) <= float(lr_max)):
        raise ValueError(f"lr_min={lr_min!r} is greater than lr_max={lr_max!r}")
    if lr_schedule == "adaptive":
        if not _finite(desired_kl, 0.0):
            raise ValueError(f"desired_kl={desired_kl!r}: lr_schedule='adaptive' needs a positive finite number")
        if not (_number(lr) and float(lr_min) <= float(lr) <= float(lr_max)):
            raise ValueError(f"lr={lr!r} starts outside [lr_min, lr_max] = [{lr_min!r}, {lr_max!r}]")
        if optimiser_steps is not None and int(optimiser_steps) < 2:
            raise ValueError(f"lr_schedule='adaptive' with {optimiser_steps} optimiser step per update: the only KL measured is taken "
                             "at the rollout's own parameters and is zero by construction")
    elif desired_kl is not None:
        raise ValueError(f"desired_kl={desired_kl!r} without lr_schedule='adaptive' would be ignored")
    return dict(lr_schedule=lr_schedule, lr_final=None if lr_final is None else float(lr_final),
                ent_beta_final=None if ent_beta_final is None else float(ent_beta_final),
                schedule_iterations=None if schedule_iterations is None else int(schedule_iterations),
                desired_kl=None if desired_kl is None else float(desired_kl), lr_factor=float(lr_factor), lr_min=float(lr_min),
                lr_max=float(lr_max))


def linear_value(start, final, k, K):
    """start + (final - start) * min(k, K) / K in f64: the value of iteration k (0-based) of a K-iteration linear schedule, held at
    `final` from iteration K on."""
    start, final = np.float64(start), np.float64(final)
    return start + (final - start) * np.float64(min(int(k), int(K))) / np.float64(K)


def fresh_state(lr):
    """The state uav_lr_init leaves: {lr, 0, 0, 0, 0, 0}."""
    s = np.zeros(STATE_N, dtype=np.float64)
    s[0] = lr
    return s


def adapt_rule(state, sums8, desired_kl, factor, lr_min, lr_max):
    """New state f64 [6] = {lr, last_kl, raised, lowered, held, skipped} after one update whose last epoch left the eight
    all-reduced sums sums8: the lines of lr_adapt_kernel, in its order of operations.  last_kl is the kl the decision saw; a
    skipped update records NaN."""
    lr, _, raised, lowered, held, skipped = (np.float64(v) for v in np.asarray(state, dtype=np.float64).reshape(STATE_N))
    S = np.asarray(sums8, dtype=np.float64).reshape(ops.PPO_DIAG_N)
    desired_kl, factor, lr_min, lr_max = (np.float64(v) for v in (desired_kl, factor, lr_min, lr_max))
    n, kl = S[7], np.float64("nan")
    q = S[1] / n if n > 0.0 else kl
    if not q == q:
        skipped = skipped + 1.0
    else:
        kl = q
        if q > 2.0 * desired_kl:
            lr = max(lr / factor, lr_min)
            lowered = lowered + 1.0
        elif q < desired_kl / 2.0:
            lr = min(lr * factor, lr_max)
            raised = raised + 1.0
        else:
            held = held + 1.0
    return np.array([lr, kl, raised, lowered, held, skipped], dtype=np.float64)


def save_state(controller, model_path):
    """The training scripts: the controller's state_dict() (plus the rule's four constants) as lr_state.npz beside the saved
    model; returns the path.  The state is the same on every rank."""
    import os
    path = os.path.join(os.path.dirname(model_path) or ".", STATE_FILE)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez(path, desired_kl=controller.desired_kl, factor=controller.factor, lr_min=controller.lr_min, lr_max=controller.lr_max,
             **controller.state_dict())
    return path


class LrController:
    """The trainer's collaborator for lr_schedule="adaptive" (like RewardNormaliser): owns the rule's state and lr_dev, the f32
    rate the Adam step reads from device memory.  adapt() is one launch; lr() is the one method that reads the host."""

    def __init__(self, lr, desired_kl, factor=1.5, lr_min=1e-6, lr_max=1e-2, device="cuda"):
        c = check_lr_control("adaptive", lr=lr, desired_kl=desired_kl, lr_factor=factor, lr_min=lr_min, lr_max=lr_max)
        self.desired_kl, self.factor, self.lr_min, self.lr_max = c["desired_kl"], c["lr_factor"], c["lr_min"], c["lr_max"]
        self.device = torch.device(device)
        self.state = torch.zeros(STATE_N, dtype=torch.float64, device=self.device)
        self.lr_dev = torch.zeros(1, dtype=torch.float32, device=self.device)
        self.reset(lr)

    def reset(self, lr):
        ops.lr_init(self.state, lr, lr_out=self.lr_dev)

    def adapt(self, diag8):
        """diag8: the all-reduced f64 [8] sums of the update's last epoch (device).  The rate of the NEXT update."""
        ops.lr_adapt(self.state, diag8, self.desired_kl, self.factor, self.lr_min, self.lr_max, lr_out=self.lr_dev)

    def lr(self):
        """The rate the next update runs with (one host read; for logs, not for the loop)."""
        return float(self.state[0].item())

    def state_dict(self):
        return {"state": self.state.cpu().numpy()}

    def load_state_dict(self, sd):
        state = np.asarray(sd["state"], dtype=np.float64).reshape(-1)
        if state.size != STATE_N:
            raise ValueError(f"lr controller state: {state.size} values, expected {STATE_N}")
        if not self.lr_min <= state[0] <= self.lr_max:
            raise ValueError(f"lr controller state: lr={state[0]!r} outside [lr_min, lr_max] = [{self.lr_min!r}, {self.lr_max!r}]")
        # the rate and its f32 form by the kernel that a fresh start uses; the other five slots behind it on the stream
        ops.lr_init(self.state, float(state[0]), lr_out=self.lr_dev)
        self.state[1:].copy_(torch.from_numpy(state[1:].copy()))
