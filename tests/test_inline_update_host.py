"""CPU: the restatement of the inline PPO update (tests/_inline_update_check.py) against the recording of the reference's
own PPOV1.1/train_ppo1.0.py run (tests/golden/update_v10.npz, tools/gen_golden_train_v10.py), a hand case of its GAE, and
its chunking against per-chunk autograd.  The GPU tests (tests/test_gpu_inline_update.py) check the kernels against this
restatement in f64, so it has to meet the reference here first."""
import numpy as np
import pytest
import torch

import _inline_update_check as iu


@pytest.fixture(scope="module")
def rec(golden):
    return golden("update_v10.npz")


def _sd(rec, i, dtype=torch.float32):
    return {k: torch.from_numpy(rec["sd." + k][i]).to(dtype).clone() for k in iu.KEYS}


def _buffer(rec, u, dtype=torch.float32):
    f = lambda k: torch.from_numpy(rec[k][u]).to(dtype)
    return f("states"), torch.from_numpy(rec["actions"][u]), f("rewards"), f("values"), f("log_probs"), f("dones")


def test_restatement_reproduces_the_reference_recording_in_f32(rec):
    """Three updates of five one-chunk epochs from the recorded initial state_dict, buffers, V(next_state) and permutations:
    every post-update state_dict to atol 4e-7 (the bound of tests/test_gpu_dropin.py for the same kind of check), every
    optimiser step's total loss to 1e-6."""
    E, B = int(rec["epochs"]), int(rec["batch_size"])
    hp = dict(gamma=float(rec["gamma"]), lam=float(rec["lam"]), clip=float(rec["clip"]), beta=float(rec["ent_beta"]))
    assert rec["perms"].shape == (3 * E, B) and rec["states"].shape == (3, B, 6)
    p = _sd(rec, 0)
    opt = iu.ClipAdam(p, lr=float(rec["lr"]))
    for u in range(3):
        perms = [torch.from_numpy(rec["perms"][u * E + e]) for e in range(E)]
        _, _, steps = iu.update(p, opt, *_buffer(rec, u), torch.tensor(rec["next_value"][u]), perms, batch_size=B, **hp)
        for e, st in enumerate(steps):
            want = rec["loss"][u * E + e]
            print("update", u, "epoch", e, "loss", st["loss"][0], "want", want, "gnorm", st["gnorm"], rec["gnorm"][u * E + e])
            assert abs(st["loss"][0] - want) <= 1e-6
            assert abs(st["gnorm"] - rec["gnorm"][u * E + e]) <= 1e-4 * rec["gnorm"][u * E + e]
        moved = []
        for k in iu.KEYS:
            err = (p[k] - torch.from_numpy(rec["sd." + k][u + 1])).abs().max().item()
            moved.append((p[k] - torch.from_numpy(rec["sd." + k][u])).abs().max().item())
            print("update", u, k, "err", err, "moved", moved[-1])
            assert err <= 4e-7, (u, k, err)
        # the update moved the tensors by far more than the bound, so agreement says something (a one-element tensor may
        # come back to where it was: the critic's bias does in the second update)
        assert sorted(moved)[1] > 1e-5 and max(moved) > 1e-4, (u, moved)


def test_the_recording_keeps_the_log_prob_clamp_inert(rec):
    p = np.exp(rec["log_probs"].astype(np.float64))
    assert p.min() >= 1e-4 and p.max() <= 1 - 1e-4
    assert rec["dones"][:, :-1].sum() >= 1                  # an episode ends inside a recorded buffer ...
    last = rec["dones"][:, -1]
    assert last.any() and not last.all()                    # ... and both branches of the last step's mask were walked by the reference


def test_gae_hand_case_pins_both_masks():
    """L = 4, gamma = 0.5, lambda = 1 (every product exact in binary), a done at t = 1 and on the last step.
    t = 3: own done -> mask 0: the bootstrap 100 must NOT enter;          A3 = 1 - 8 = -7
    t = 2: mask 1 - done[3] = 0;                                          A2 = 1 - 4 = -3
    t = 1: mask 1 - done[2] = 1 (its OWN done[1] = 1 is not its mask);    A1 = 1 + .5 * 4 - 2 + .5 * -3 = -0.5
    t = 0: mask 1 - done[1] = 0;                                          A0 = 1 - 1 = 0
    and with the last done cleared the bootstrap enters: A3 = 1 + 50 - 8 = 43, A2 = 1 + 4 - 4 + .5 * 43 = 22.5, ..."""
    rew, val = torch.ones(4, dtype=torch.float64), torch.tensor([1.0, 2.0, 4.0, 8.0], dtype=torch.float64)
    done = torch.tensor([0.0, 1.0, 0.0, 1.0], dtype=torch.float64)
    adv = iu.gae_inline(rew, val, done, 100.0, gamma=0.5, lam=1.0)
    assert adv.tolist() == [0.0, -0.5, -3.0, -7.0]
    done[3] = 0.0
    adv = iu.gae_inline(rew, val, done, 100.0, gamma=0.5, lam=1.0)
    assert adv.tolist() == [0.0, 1.0 + 2.0 - 2.0 + 0.5 * 22.5, 22.5, 43.0]
    # [n, T] rows are independent, next_value per row
    both = iu.gae_inline(rew.repeat(2, 1), val.repeat(2, 1), torch.stack([done, done]), torch.tensor([100.0, 0.0]).double(), 0.5, 1.0)
    assert both[0].tolist() == adv.tolist() and both[1, 3].item() == 1.0 - 8.0
    a_n, ret = iu.normalise_inline(adv, val)
    assert torch.equal(ret, adv + val) and abs(a_n.mean().item()) < 1e-15 and abs(a_n.std().item() - 1) < 1e-7
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")        # torch warns about the degrees of freedom; the NaN is the point
        assert torch.isnan(iu.normalise_inline(adv[:1], val[:1])[0]).all()


def test_chunked_epochs_are_per_chunk_autograd(rec):
    """B = 100 < L = 256: three chunks per epoch, the last of 56 rows; every step's gradient is autograd's on exactly that
    chunk at the parameters the steps before it left, with means over the chunk's own length."""
    p = _sd(rec, 0, torch.float64)
    buf = _buffer(rec, 0, torch.float64)
    g = torch.Generator().manual_seed(3)
    perms = [torch.randperm(256, generator=g) for _ in range(2)]
    opt = iu.ClipAdam(p, lr=1e-3)
    adv_n, ret, steps = iu.update(p, opt, *buf, torch.tensor(rec["next_value"][0]).double(), perms, batch_size=100)
    assert [s["n"] for s in steps] == [100, 100, 56] * 2
    states, actions, _, values, log_probs, _ = buf
    q = _sd(rec, 0, torch.float64)
    opt2 = iu.ClipAdam(q, lr=1e-3)
    for i, st in enumerate(steps):
        idx = perms[i // 3][(i % 3) * 100:(i % 3) * 100 + 100]
        leaf = {k: v.clone().requires_grad_(True) for k, v in q.items()}
        probs, value = iu.forward(leaf, states[idx])
        total = iu.losses(probs, value, actions[idx], log_probs[idx], adv_n[idx], ret[idx], values[idx])[0]
        total.backward()
        for k in iu.KEYS:
            assert torch.equal(st["params"][k], q[k]) and torch.equal(st["grad"][k], leaf[k].grad), (i, k)
        assert st["loss"][0] == float(total.detach())
        opt2.step(q, {k: leaf[k].grad for k in q})
    for k in iu.KEYS:
        assert torch.equal(p[k], q[k])


def test_trainer_arguments_are_checked_before_anything_is_built():
    """No device is touched before these checks (they run on a host without a GPU)."""
    from uavppo import ops
    from uavppo.trainer import VecPPOTrainer
    assert ops.GAE_MODES == {"reference_exact": 0, "standard": 1, "inline_v10": 2}
    with pytest.raises(ValueError, match="MLP policy on the fused path"):
        VecPPOTrainer(8, 32, "lstm", hidden=64, minibatch_rows=100)
    with pytest.raises(ValueError, match="give one of them"):
        VecPPOTrainer(8, 32, "mlp", minibatch_rows=100, num_minibatches=2)
    with pytest.raises(ValueError, match="positive row count"):
        VecPPOTrainer(8, 32, "mlp", minibatch_rows=0)
    with pytest.raises(ValueError, match="update_form"):
        VecPPOTrainer(8, 32, "mlp", update_form="inline")
    with pytest.raises(ValueError, match="gae_mode='standard' would be ignored"):
        VecPPOTrainer(8, 32, "mlp", update_form="inline_v10", gae_mode="standard")
