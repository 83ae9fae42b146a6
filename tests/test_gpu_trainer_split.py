"""VecPPOTrainer's two collaborators on the GPU: the mirror ring both share (uavppo/mirror_ring.py), the curriculum link with
the host more than a ring ahead of its reads (uavppo/curriculum_link.py), and the range guard's one decide-and-set path
reached from a rollout and from an update (uavppo/range_guard.py).  -m gpu."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def test_mirror_ring_under_the_guards_overflow_policy():
    """Six rows into four slots without a poll in between; before the fifth and the sixth push the range guard's policy -- wait
    for the oldest slot, poll -- makes room.  Once everything has landed one poll returns the slot of the sixth row and empties
    the ring."""
    from uavppo.mirror_ring import MirrorRing
    ring = MirrorRing((3,), torch.float32, slots=4)
    rows = (torch.arange(18, dtype=torch.float32, device=DEV) + 1.0).view(6, 3)
    for i in range(6):
        if len(ring) == ring.slots:
            assert i >= 4
            oldest = ring.oldest
            assert torch.equal(ring.wait(oldest), rows[oldest].cpu())      # slots 0, 1 still hold rows 0, 1 when they are waited for
            assert ring.poll() is not None
        assert ring.push(rows[i]) == i % 4
        assert 1 <= len(ring) <= 4
    torch.cuda.synchronize()
    slot = ring.poll()
    assert slot == 5 % 4 and torch.equal(ring.host[slot], rows[5].cpu())
    assert ring.poll() is None and len(ring) == 0


def test_device_curriculum_with_the_host_more_than_a_ring_ahead():
    """Six iterations -- more than the four mirror slots -- without one curriculum read on the device trainer: the link drops the
    mirrors it overwrites, and what is read afterwards equals the host curriculum's run on the same seed; the last mirror holds
    the episode count from before the sixth rollout."""
    from uavppo.trainer import VecPPOTrainer
    mk = lambda device: VecPPOTrainer(64, 16, "lstm", hidden=64, device=DEV, seed=5, device_curriculum=device)
    dev, host = mk(True), mk(False)
    for tr in (dev, host):
        tr.radius = 200.0            # episodes end in every rollout
        tr.reset()
    host.curriculum.current_radius = 200.0
    assert dev.device_curriculum and not host.device_curriculum
    for _ in range(6):
        dev.train_iteration()
    slot = dev.last_mirror_slot
    for it in range(6):
        if it == 5:
            before_sixth = host.episodes_done
        host.train_iteration()
    assert len(dev.link.ring) <= dev.link.ring.slots
    got = dev.episodes_before_rollout(slot)
    print("episodes before the sixth rollout:", got, before_sixth, " done:", dev.episodes_done, host.episodes_done,
          " successes:", dev.successes_done, host.successes_done, " radius:", dev.radius, host.radius, " bonus:", dev.bonus, host.bonus)
    assert got == before_sixth
    assert dev.radius == host.radius and dev.bonus == host.bonus
    assert dev.episodes_done == host.episodes_done and dev.successes_done == host.successes_done
    assert 0 < before_sixth < host.episodes_done         # (the comparison is about episodes that ended, in the sixth rollout too)


def test_range_guard_decides_the_same_before_a_rollout_and_before_an_update():
    """One weight above half the fp16 limit, written before a collect() on one trainer and between collect() and update() on
    another: both entries of the guard measure it, count one event and set the bf16-split kernels on the handle; with the weight
    restored the next iteration is back on the fp16 split."""
    from uavppo import ops
    from uavppo.trainer import VecPPOTrainer
    mk = lambda: VecPPOTrainer(32, 8, "lstm", hidden=64, device=DEV, seed=3, epochs=1)

    def put(tr, v):
        with torch.no_grad():
            tr.policy.views["lstm.weight_hh_l0"][5, 7] = v

    a = mk()
    put(a, 1.0e5)
    a.collect()
    assert a.arith == "bf16x6" and a.range_events == 1
    a.update()
    assert a.arith == "bf16x6" and a.range_events == 1 and ops.get_lstm_arith(DEV) == "bf16x6"
    b = mk()
    b.collect()
    assert b.arith == "fp16x3" and b.range_events == 0 and ops.get_lstm_arith(DEV) == "fp16x3"
    put(b, 1.0e5)
    b.update()
    assert b.arith == "bf16x6" and b.range_events == 1 and ops.get_lstm_arith(DEV) == "bf16x6"
    for tr in (a, b):
        tr.update_curriculum()
        tr.iteration += 1
        put(tr, 0.01)
        tr.train_iteration()
        assert tr.arith == "fp16x3" and ops.get_lstm_arith(DEV) == "fp16x3"
        assert np.isfinite(tr.losses()).all() and torch.isfinite(tr.policy.flat).all()
