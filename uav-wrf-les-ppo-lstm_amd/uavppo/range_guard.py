"""RangeGuard: keeps the fp16-split kernels inside their operand ranges without stalling the training loop.

The fp16-split kernels need |w| < 65504, |x| < 4096, |h0| < 64 (include/uavppo.h).  What can leave that range, and
where it is caught without stalling the loop:
  parameters   move by <= lr per optimiser step.  The Adam kernel publishes max |param| after every step
               (uav_clip_adam's pmax_out, written to `ranges[0:1]`); its copy to pinned host memory is polled, never waited
               for, at the start of a later rollout (the host runs one to two iterations ahead of the device), against HALF
               the limit.  Parameters written by anything else (initialisation, load_state_dict: torch bumps flat._version)
               are measured before the next rollout runs on them -- a sync, on such an iteration only.
  observations / recurrent state of the trainer's OWN rollouts are bounded by construction (positions, field values
               and counters scaled to O(1); |h| < 1), so they are not measured in the loop.  Buffers filled by a
               caller (update() without a preceding collect()) ARE measured, synchronously, before the update.
"""
import torch

from . import ops
from .mirror_ring import MirrorRing

# operand ranges of the default (fp16-split) LSTM kernels, include/uavppo.h: |w| < 65504, |x| < 4096, |h0| < 64.  The
# trainer switches to the bf16-split kernels at HALF of each limit; parameters move by at most lr per optimiser step, so a
# weight maximum read one iteration late still has that margin.
RANGE_LIMITS = (0.5 * 65504.0, 0.5 * 4096.0, 0.5 * 64.0)
# the fused MLP kernels run their 256 x 128 products on the same fp16 split: its operand a1 = relu(LayerNorm) is bounded by
# sqrt(255) |g1| + |be1|, so max |param| < 2048 keeps it inside fp16's range (include/uavppo.h, uav_mlp_ppo_grad); half of it:
MLP_RANGE_LIMITS = (0.5 * 2048.0, float("inf"), float("inf"))


class RangeGuard:
    def __init__(self, policy, kind, device, enabled):
        """enabled: every LSTM policy -- the h = 64 / 128 sequence kernels AND the h = 256 step kernels are fp16-split by default
        (at h = 256 the wide-range modes run the generic exact-f32 step path -- slow, but never silently out of range) -- and
        the fused MLP kernels likewise (their wide-range mode is the exact-f32 MFMA form of the same kernels)."""
        self.policy, self.kind, self.device, self.enabled = policy, kind, device, bool(enabled)
        self.limits = RANGE_LIMITS if kind == "lstm" else MLP_RANGE_LIMITS
        # device maxima [|param|, |obs|, |h0|], mirrored to pinned host memory (a ring: the host may run iterations ahead)
        self.ranges = torch.zeros(3, dtype=torch.float32, device=device)
        self.ring = MirrorRing((3,), torch.float32)     # in flight: copies of the Adam kernel's max |param|
        self.buffers_own = False     # True between a rollout and the update that consumes its buffers
        self.arith = "fp16x3"
        self.range_events = 0        # iterations that ran on the wide-range (bf16-split) kernels
        # force_arith: "fp16x3" | "bf16x6" | "f32_mfma" pins the LSTM kernels' arithmetic (A/B runs, reference gradients);
        # None = the range guard decides.  A handle that uav_create started in another mode (UAV_LSTM_F32_MFMA=1 /
        # UAV_LSTM_BF16X6=1 in the environment: a whole-process A/B) keeps it.
        init_mode = ops.Context.get(device).initial_arith
        self.force_arith = None if init_mode == "fp16x3" else init_mode
        self.flat_version = -1

    def _decide(self, maxima):
        ok = all(v == v and v < lim for v, lim in zip(maxima, self.limits))
        self.arith = "fp16x3" if ok else "bf16x6"
        self.range_events += (not ok)
        if self.force_arith is not None:
            self.arith = self.force_arith
        return ok

    def _settle(self, own, obs=None, h0=None):
        """Force, decide, set the handle's arithmetic.  Own buffers: the parameters are probed (synchronously) only when
        something other than the Adam kernel wrote them; foreign buffers: everything is measured now."""
        if self.force_arith is not None:
            self.arith = self.force_arith
        flat = self.policy.flat
        if not own or flat._version != self.flat_version:
            self.ring.clear()                   # maxima published before the foreign write say nothing about it
            ops.absmax(flat, out=self.ranges[0:1])
            if not own and self.kind == "lstm":
                ops.absmax(obs, out=self.ranges[1:2])
                ops.absmax(h0, out=self.ranges[2:3])
            self.flat_version = flat._version
            self._decide([float(self.ranges[0].item()), 0.0, 0.0] if own else self.ranges.tolist())
        ops.set_lstm_arith(self.arith, self.device)

    def before_rollout(self):
        """Kernel arithmetic for the rollout about to be queued, whose buffers are then the trainer's own."""
        if self.enabled:
            self.poll()
            self._settle(own=True)
            self.buffers_own = True

    def before_update(self, obs, h0):
        """Kernel arithmetic for the update about to be queued (see above); sets it on the device's handle."""
        if self.enabled:
            self._settle(self.buffers_own, obs, h0)
        return self.arith

    def after_update(self):
        """max |param| of the last Adam step -> pinned host memory, read at a later poll."""
        if not self.enabled:
            return
        if len(self.ring) == self.ring.slots:     # the host is four updates ahead of the device: let the oldest copy land
            self.ring.wait(self.ring.oldest)
            self.poll()
        self.ring.push(self.ranges)
        self.buffers_own = False

    def poll(self):
        """Read the newest of the Adam kernel's max |param| copies that has landed (never waits)."""
        latest = self.ring.poll()
        if latest is not None and self.enabled:
            self._decide([float(self.ring.host[latest, 0]), 0.0, 0.0])
