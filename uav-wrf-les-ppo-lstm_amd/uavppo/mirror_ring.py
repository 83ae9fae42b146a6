"""MirrorRing: lagged host mirrors of a small device block.  The host may run iterations ahead of the device, so a block it
wants to read without waiting is copied to the next of a few pinned slots, an event is recorded behind the copy, and a later
poll takes the newest slot whose copy has landed.  What happens when the host is a whole ring ahead -- wait for the oldest
slot, or drop it -- is the caller's policy (uavppo/range_guard.py, uavppo/curriculum_link.py)."""
import torch


class MirrorRing:
    def __init__(self, shape, dtype, slots=4):
        self.host = torch.zeros((slots,) + tuple(shape), dtype=dtype).pin_memory()
        self.events = [torch.cuda.Event() for _ in range(slots)]
        self.in_flight = []          # slots whose copy is on its way, oldest first
        self.next = 0                # the slot the next push() writes

    def __len__(self):
        return len(self.in_flight)

    @property
    def slots(self):
        return len(self.events)

    @property
    def oldest(self):
        return self.in_flight[0]

    def clear(self):
        self.in_flight.clear()

    def push(self, src, stream=None):
        """Copy src to the next slot without blocking and record the slot's event behind it (on `stream`; None = the current one)."""
        k = self.next
        self.next = (k + 1) % self.slots
        self.host[k].copy_(src, non_blocking=True)
        self.events[k].record(stream)
        self.in_flight.append(k)
        return k

    def poll(self):
        """Pop every slot whose copy has landed; the newest of them, or None (never waits)."""
        latest = None
        while self.in_flight and self.events[self.in_flight[0]].query():
            latest = self.in_flight.pop(0)
        return latest

    def wait(self, slot):
        """Host row of `slot`, after waiting for that slot's copy only."""
        self.events[slot].synchronize()
        return self.host[slot]
