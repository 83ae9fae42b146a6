"""CurriculumLink: a rollout's success flags on their way to the curriculum, and the curriculum's radius / bonus on their way
back to the environments.

device_curriculum (the default with a curriculum): the 120-episode window, radius and bonus live in a device block
(uav_curriculum_*), updated by a one-thread kernel on the side stream from the gathered success messages and read by
the env kernels at launch -- the loop has no host synchronisation left.  False: the host-side Curriculum class (the
reference's arithmetic in Python; what the N = 1 PPOTrainer of model.py uses), one wait per iteration.

radius / bonus / episode counters.  Host curriculum: plain attributes.  Device curriculum: the truth is on the device; the
`radius`, `bonus`, `episodes_done`, `successes_done` getters WAIT for it (tests, logging at the end of a run); the training
loop itself never calls them -- it reads the lagged mirror (`radius_lagged`, `episodes_lagged`: the state as of the rollout
before last, copied to pinned memory on the side stream).

A rollout's flags (`stage`): packed right behind the rollout on the side stream; exchanged from after_rollout() with one rank,
with collectives on from in_update() behind the advantage-statistics all-reduce (or from count() if still outstanding);
counted by count().  _IDLE: use_side_stream = False, or buffers a caller filled by hand.
"""
import numpy as np
import torch

from . import ops
from .curriculum import Curriculum
from .dist_utils import SUCC_CAP, abi_collectives, exchange_successes, pack_local_successes, unpack_episode_successes
from .mirror_ring import MirrorRing

_SIDE_STREAMS = {}


def _side_stream(device):
    """ONE side stream per device and process, shared by every trainer built in it.  A trainer used to draw its own
    stream from torch's pool; a SECOND trainer in a process (bench.py's old weak -> strong sequence) then ran its success
    exchange on a second pool stream, and with two rank processes sharing one GPU over gloo every iteration of that second
    trainer stalled for 50-900 ms in update() (tools/two_phase_probe.py: `base` 58-245 ms per C3 iteration against 9.6 ms
    in fresh processes; `samestream` -- the second trainer reusing the first one's stream -- 10.7 ms; `nocurr` and
    `mainstream`, which never touch a side stream, 9.0 / 9.8 ms; dropping the first trainer, gc, empty_cache, kernel
    timers and the torch thread count made no difference).  Streams are a per-process resource: keep exactly one."""
    device = torch.device(device)
    key = device.index if device.index is not None else torch.cuda.current_device()
    if key not in _SIDE_STREAMS:
        _SIDE_STREAMS[key] = torch.cuda.Stream(device=device)
    return _SIDE_STREAMS[key]


# CurriculumLink.stage, where the buffers' success flags are: not packed | packed (side stream) | gathered and handed on | counted
_IDLE, _PACKED, _EXCHANGED, _COUNTED = range(4)


class _DeviceCurriculumView:
    """What callers read off `trainer.curriculum` when the curriculum lives on the device (each access waits for the device)."""

    def __init__(self, link):
        self._link = link

    @property
    def current_radius(self):
        return self._link.radius

    @property
    def explore_bonus(self):
        return self._link.bonus

    @property
    def success_history(self):
        self._link.sync()
        return [None] * self._link.hist_len         # the window's LENGTH is what callers look at; its bits stay on the device


class CurriculumLink:
    def __init__(self, device, world, coll, use_curriculum=True, device_curriculum=None):
        self.device, self.world, self._coll = torch.device(device), int(world), bool(coll)     # coll: the exchange is a collective
        self.device_curriculum = bool(use_curriculum) if device_curriculum is None else bool(device_curriculum and use_curriculum)
        self.host_radius, self.host_bonus = 50.0, 0.6
        self.episodes = self.successes = 0       # finished episodes of the whole job (all ranks)
        self.hist_len = 0
        self.last_success_bits = None
        if self.device_curriculum:
            self.block = ops.curriculum_state(self.device, self.host_radius, self.host_bonus)
            self.ring = MirrorRing((self.block.numel(),), torch.uint8)       # lagged host mirrors of the block
            self.last_mirror_slot = 0
            self._done_ev = torch.cuda.Event()   # behind the side stream's last update of the block
            self._pending = False
            self.curriculum = _DeviceCurriculumView(self)
        else:
            self.block = None
            self.curriculum = Curriculum() if use_curriculum else None
        # the curriculum's success bits leave on a side stream right behind the rollout and land in pinned host memory
        # while the update runs: the iteration's one host sync (count) then waits for a copy that finished
        # milliseconds ago instead of draining the main stream
        self.side = _side_stream(self.device) if use_curriculum else None
        self._succ_host = (torch.zeros(self.world, 4 + SUCC_CAP + 1, dtype=torch.uint8).pin_memory() if use_curriculum else None)
        self._succ_ev = torch.cuda.Event()
        self._pack_ev = torch.cuda.Event()
        self._roll_ev = torch.cuda.Event()
        self._gather_ev = torch.cuda.Event()
        self.stage = _IDLE                     # where the flags of the current buffers are on their way to the curriculum
        self._msg = None
        self.use_side_stream = True            # False: pack + copy on the main stream inside count() (A/B, tools/ab_loop.py)
        self._rollout_radius = self.host_radius

    # ------------------------------------------------------------------------------------------ reads
    def _read(self, block, adopt=True):
        """A HOST copy of the device curriculum block -> its scalars, taken as this link's own unless adopt=False.  An overflowed
        message raises wherever the block is read: through the mirror one or two rollouts late, never at the end of a long run only."""
        d = ops.curriculum_read(block.numpy())
        if d["overflow"]:
            raise RuntimeError(f"device curriculum: a rank ended more than {SUCC_CAP} episodes in one rollout (message capacity)")
        if adopt:
            self.host_radius = d["radius"]
            self.host_bonus = np.float64(d["bonus"]) if d["bonus_is_f64"] else d["bonus"]
            self.episodes, self.successes, self.hist_len = d["episodes"], d["successes"], d["hist_len"]
        return d

    def _read_mirror_slot(self, k):
        return self._read(self.ring.wait(k), adopt=False)        # waits for that 64-byte copy only

    def sync(self):
        """Device curriculum: wait for the device state and take it as the host scalars."""
        if not self.device_curriculum:
            return
        if self.stage == _PACKED and not self._coll:
            self._exchange()                   # (with several ranks the exchange is a collective: only in_update() / before_rollout() issue it)
        if self._pending:
            self._done_ev.synchronize()
        self._read(self.block.cpu())

    def _poll_mirror(self):
        """Newest landed mirror of the device state (never waits; the host curriculum queues none)."""
        if self.device_curriculum:
            latest = self.ring.poll()
            if latest is not None:
                self._read(self.ring.host[latest])

    def rollout_radius(self, k=None):
        """The radius the LAST collected rollout ran with (device curriculum: from its lagged mirror, slot k = the value of
        `last_mirror_slot` taken right after that rollout's count(); waits only for that 64-byte copy)."""
        return self._read_mirror_slot(self.last_mirror_slot if k is None else k)["radius"] if self.device_curriculum else self._rollout_radius

    def episodes_before_rollout(self, k):
        """Episodes the whole job had finished BEFORE the rollout whose mirror went to slot k (its `last_mirror_slot`): waits for
        that 64-byte copy only.  The mirror is taken on the device between two curriculum updates, from state every rank holds
        identically -- so this value, unlike the polled `episodes_lagged`, is the same on every rank at the same program point:
        what a multi-rank loop must base its stop decision on (a rank that stops alone leaves the others in the next all-reduce)."""
        return self._read_mirror_slot(k)["episodes"] if self.device_curriculum else self.episodes

    @property
    def radius(self):
        self.sync()
        return self.host_radius

    def _before_host_write(self):
        """A host-side write into the device block must land behind the side stream's pending update of it."""
        if self._pending:
            torch.cuda.current_stream().wait_event(self._done_ev)

    @radius.setter
    def radius(self, v):
        self.host_radius = float(v)
        if self.device_curriculum:
            self._before_host_write()
            self.block[:32].view(torch.float64)[0] = self.host_radius

    @property
    def bonus(self):
        self.sync()
        return self.host_bonus

    @bonus.setter
    def bonus(self, v):
        self.host_bonus = v
        if self.device_curriculum:
            self._before_host_write()
            self.block[:32].view(torch.float64)[1] = float(v)
            self.block[:32].view(torch.float64)[2] = 1.0 if isinstance(v, np.float64) else 0.0

    @property
    def radius_lagged(self):
        self._poll_mirror()
        return self.host_radius

    @property
    def episodes_lagged(self):
        self._poll_mirror()
        return self.episodes

    @property
    def episodes_done(self):
        self.sync()
        return self.episodes

    @property
    def successes_done(self):
        self.sync()
        return self.successes

    # ------------------------------------------------------------------------------------------ successes -> curriculum
    def before_rollout(self):
        self._rollout_radius = self.host_radius    # (host curriculum: what this rollout runs with)
        if self.stage in (_PACKED, _EXCHANGED):    # a previous rollout's flags may still be read by the pack kernel on the side stream
            torch.cuda.current_stream().wait_event(self._pack_ev)
        if self.device_curriculum:
            if self.stage == _PACKED:          # a rollout twice without an update: finish the first one's exchange
                self._exchange()
            if self._pending:                  # the env kernels read radius / bonus from the device state: a GPU-side wait, no host sync
                torch.cuda.current_stream().wait_event(self._done_ev)
        self.stage = _IDLE

    def after_rollout(self, flags):
        """Pack the rollout's flags on the side stream; with one rank, exchange them at once."""
        if self.curriculum is not None and self.use_side_stream:
            self._pack(flags)
            if not self._coll:
                self._exchange()

    def in_update(self):
        """With collectives on: the exchange, where update() stands behind the advantage-statistics all-reduce."""
        if self.stage == _PACKED:
            self._exchange()

    def _pack(self, flags):
        self._roll_ev.record()
        with torch.cuda.stream(self.side):
            self.side.wait_event(self._roll_ev)
            self._msg = pack_local_successes(flags)
            self._pack_ev.record(self.side)        # the flags have been read: the next rollout may overwrite them
        self.stage = _PACKED

    def _gather(self, msg):
        msgs = exchange_successes(msg)
        if tuple(msgs.shape) != tuple(self._succ_host.shape):       # e.g. world_size > 1 without a process group
            raise RuntimeError(f"success exchange returned {tuple(msgs.shape)}, expected {tuple(self._succ_host.shape)}: "
                               "is torch.distributed initialised for world_size > 1?")
        return msgs

    def _exchange(self):
        """All-gather of the packed success bits + copy to pinned host memory, on the side stream.  With several ranks it is
        issued from update(), BEHIND the advantage-statistics all-reduce in program order: RCCL runs a rank's collectives
        in the order they were issued, and that all-reduce must not queue behind the pack kernel."""
        on_main = abi_collectives() and self._coll
        if on_main:
            # ABI carrier: ONE communicator on raw streams.  RCCL runs a rank's collectives in the order its device reaches them, so
            # the all-gather must not sit on another stream than the all-reduces (two ranks could then reach the two collectives in
            # opposite orders and wait for each other): it goes on the MAIN stream, behind the pack kernel, and the side stream
            # picks the gathered messages up again.  (torch.distributed serialises a group's collectives on its own stream.)
            main = torch.cuda.current_stream()
            main.wait_event(self._pack_ev)
            msgs = self._gather(self._msg)
            self._gather_ev.record(main)
        with torch.cuda.stream(self.side):
            if on_main:
                self.side.wait_event(self._gather_ev)
            else:
                msgs = self._gather(self._msg)
            if self.device_curriculum:
                # lagged host mirror of the state as it was for THIS rollout, then the update itself: one thread walks the
                # messages rank by rank, episode by episode (model.py:131-164)
                if self.ring.next in self.ring.in_flight:       # the host is a whole ring ahead: drop the oldest mirror
                    self.ring.in_flight.remove(self.ring.next)
                self.last_mirror_slot = self.ring.push(self.block, self.side)
                ops.curriculum_update(self.block, msgs, SUCC_CAP)
                self._done_ev.record(self.side)
                self._pending = True
            else:
                self._succ_host.copy_(msgs, non_blocking=True)
                self._succ_ev.record(self.side)
        self.stage = _EXCHANGED

    def count(self, flags):
        """Feed this iteration's finished episodes to the curriculum (host scalars).  The success bits are
        compacted on the device; only they cross to the host / the other ranks, so every rank feeds the same
        global (env, time)-ordered sequence to its replicated curriculum.  A rollout's episodes are counted once: a second
        call before the next rollout does nothing."""
        if self.curriculum is None or self.stage == _COUNTED:
            return
        if self.stage == _IDLE and self.device_curriculum:          # flags not produced by a rollout: pack them now
            self._pack(flags)
        if self.stage == _IDLE:                # host curriculum: pack and exchange them now, on the main stream
            self._succ_host.copy_(self._gather(pack_local_successes(flags)), non_blocking=True)
            self._succ_ev.record()
        elif self.stage == _PACKED:            # a rollout without an update in between
            self._exchange()
        self.stage = _COUNTED
        if self.device_curriculum:             # no host wait: the messages were (or are now) queued, the device does the rest
            self._poll_mirror()
            return
        self._succ_ev.synchronize()
        bits = unpack_episode_successes(self._succ_host.numpy(), flags)
        self.episodes += int(bits.size)                  # over ALL ranks, in global (env, time) order
        self.successes += int(bits.sum())
        self.last_success_bits = bits
        self.curriculum.update_many(bits)
        self.host_radius, self.host_bonus = self.curriculum.current_radius, self.curriculum.explore_bonus
