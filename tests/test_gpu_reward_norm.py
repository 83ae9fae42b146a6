"""Running return-based reward normalisation on the GPU: the three kernels of csrc/reward_norm.hip through uavppo.ops against the
sequential numpy definitions of uavppo/reward_norm.py (return_traces, merge_running), RewardNormaliser inside VecPPOTrainer and
GAILTrainer, and its state_dict round trip.  -m gpu.

Bars.  Traces: 1e-12 * max(1, max |G|) -- the wave scan only reassociates at most T f64 products and sums of about 1e-16 relative
each.  stats3: 1e-11 relative to sum |G| and to sum G^2.  Merge: 1e-14 relative on the state (the kernel and merge_running run
the same f64 operations in the same order; sqrt and the division may differ in the last place), 1 ulp of f32 on the scale.
Scale: bit-equal to numpy's f32 product and clip."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(1, 1), (3, 5), (5, 64), (4, 65), (7, 130), (64, 128)]       # the chunk edges of the 64-lane scan; more than one block


@pytest.fixture(scope="module")
def ops():
    from uavppo import ops as o
    return o


def dev(x, dtype=None):
    t = torch.as_tensor(x)
    return (t if dtype is None else t.to(dtype)).to(DEV).contiguous()


def _inputs(N, T, seed):
    """Random rewards, done with p = 0.1; where the shape has the rows for it: a row that ends at step 0, one that ends at
    T - 1, one that never ends.  A non-zero carry-in."""
    rng = np.random.default_rng(seed)
    rew = (rng.standard_normal((N, T)) * 3.0 + 0.5).astype(np.float32)
    done = (rng.random((N, T)) < 0.1).astype(np.float32)
    if N >= 3:
        done[0, 0] = 1.0
        done[1, T - 1] = 1.0
        done[2, :] = 0.0
    carry = rng.standard_normal(N) * 5.0 + 1.0
    return rew, done, carry


def _run(ops, rew, done, carry, gamma, want_trace=True):
    N, T = rew.shape
    c = dev(carry, torch.float64).clone()
    tr = torch.full((N, T), float("nan"), dtype=torch.float64, device=DEV) if want_trace else None
    s3 = ops.return_stats(dev(rew), dev(done), c, gamma, trace_out=tr)
    return (None if tr is None else tr.cpu().numpy()), c.cpu().numpy(), s3.cpu().numpy()


def _ulp32(a, b):
    """Distance of two f32 values of one sign in units in the last place."""
    return abs(int(np.float32(a).view(np.int32)) - int(np.float32(b).view(np.int32)))


# ------------------------------------------------------------------------------------------------ 1: traces, carry, stats
@pytest.mark.parametrize("gamma", [0.99, 0.0])
@pytest.mark.parametrize("N,T", SHAPES)
def test_traces_carry_and_stats_against_the_sequential_definition(ops, N, T, gamma):
    from uavppo.reward_norm import return_traces
    rew, done, carry = _inputs(N, T, 100 * N + T)
    G, c_ref = return_traces(rew, done, gamma, carry)
    got, c, s3 = _run(ops, rew, done, carry, gamma)
    bar = 1e-12 * max(1.0, np.abs(G).max())
    e_tr, e_c = np.abs(got - G).max(), np.abs(c - c_ref).max()
    e_s, e_q = abs(s3[0] - G.sum()) / np.abs(G).sum(), abs(s3[1] - (G * G).sum()) / (G * G).sum()
    print(f"N={N} T={T} gamma={gamma}: trace {e_tr:.3g} carry {e_c:.3g} (bar {bar:.3g}) sum {e_s:.3g} sumsq {e_q:.3g} (bar 1e-11)")
    assert e_tr <= bar and e_c <= bar
    assert e_s <= 1e-11 and e_q <= 1e-11 and s3[2] == float(N * T)
    if gamma == 0.0:
        assert np.array_equal(got, rew.astype(np.float64))
    # without the trace buffer: the same sums and carry; and a second call on the same inputs: the same bits
    _, c2, s32 = _run(ops, rew, done, carry, gamma, want_trace=False)
    got3, c3, s33 = _run(ops, rew, done, carry, gamma)
    assert np.array_equal(s32, s3) and np.array_equal(c2, c)
    assert np.array_equal(s33, s3) and np.array_equal(c3, c) and np.array_equal(got3, got)


def test_split_invariance_on_the_device(ops):
    from uavppo.reward_norm import return_traces
    rew, done, carry = _inputs(6, 128, 7)
    done[3, 47] = 1.0                # an episode that ends exactly at the cut
    G, c_ref = return_traces(rew, done, 0.99, carry)
    whole, c_whole, _ = _run(ops, rew, done, carry, 0.99)
    a, c_a, _ = _run(ops, rew[:, :48].copy(), done[:, :48].copy(), carry, 0.99)
    b, c_b, _ = _run(ops, rew[:, 48:].copy(), done[:, 48:].copy(), c_a, 0.99)
    bar = 1e-12 * max(1.0, np.abs(G).max())
    assert c_a[3] == 0.0
    assert np.abs(np.concatenate([a, b], 1) - whole).max() <= bar and np.abs(c_b - c_whole).max() <= bar
    assert np.abs(np.concatenate([a, b], 1) - G).max() <= bar and np.abs(c_b - c_ref).max() <= bar


def test_the_calls_refuse_what_the_header_says_they_refuse(ops):
    rew, done, carry = (dev(x) for x in _inputs(3, 5, 1))
    carry = carry.to(torch.float64)
    for gamma in (-0.1, 1.5, float("nan")):
        with pytest.raises(RuntimeError):
            ops.return_stats(rew, done, carry, gamma)
    state, s3 = torch.zeros(4, dtype=torch.float64, device=DEV), torch.ones(3, dtype=torch.float64, device=DEV)
    for eps in (0.0, -1e-8, float("nan")):
        with pytest.raises(RuntimeError):
            ops.return_norm_merge(state, s3, eps)
    assert state.cpu().tolist() == [0.0] * 4            # a refused call launches nothing


# ------------------------------------------------------------------------------------------------ 3: merge
def _merge_close(got_state, got_scale, ref_state, ref_scale):
    for g, r in zip(got_state, ref_state):
        assert abs(g - r) <= 1e-14 * abs(r), (got_state, ref_state)
    assert _ulp32(got_scale, ref_scale) <= 1, (got_scale, ref_scale)


def test_merge_three_batches_against_merge_running(ops):
    from uavppo.reward_norm import batch_stats, merge_running, return_traces
    rng = np.random.default_rng(21)
    state = torch.zeros(4, dtype=torch.float64, device=DEV)
    ref, carry, eps = np.zeros(4), np.zeros(5), 1e-8
    for T in (30, 64, 9):
        rew = (rng.standard_normal((5, T)) * 2.0 - 1.0).astype(np.float32)
        done = (rng.random((5, T)) < 0.1).astype(np.float32)
        G, carry = return_traces(rew, done, 0.99, carry)
        s3 = batch_stats(G)
        scale = ops.return_norm_merge(state, dev(s3), eps)
        ref, ref_scale = merge_running(ref, s3, eps)
        _merge_close(state.cpu().numpy(), scale.item(), ref, ref_scale)
    assert ref[2] == 5.0 * (30 + 64 + 9) and ref[3] == 0.0 and ref_scale != 1.0


def test_merge_edge_cases(ops):
    from uavppo.reward_norm import merge_running
    f64 = dict(dtype=torch.float64, device=DEV)
    # count == 0 and a batch that is skipped (a NaN written here, into stats3): scale 1, one skip, nothing else moves
    state = torch.zeros(4, **f64)
    scale = ops.return_norm_merge(state, torch.tensor([float("nan"), 1.0, 10.0], **f64))
    assert scale.item() == 1.0 and state.cpu().tolist() == [0.0, 0.0, 0.0, 1.0]
    # zero variance: a constant batch passes unscaled, never divided by sqrt(eps)
    state = torch.zeros(4, **f64)
    scale = ops.return_norm_merge(state, torch.tensor([2.5 * 27, 2.5 * 2.5 * 27, 27.0], **f64))
    assert scale.item() == 1.0 and state.cpu().tolist() == [2.5, 0.0, 27.0, 0.0]
    # a running estimate survives non-finite batches: state as it was, skipped counted, the scale restated from the state
    good = np.array([12.0, 900.0, 40.0])
    state = torch.zeros(4, **f64)
    scale0 = ops.return_norm_merge(state, dev(good)).item()
    before = state.cpu().numpy()
    ref, ref_scale = merge_running(np.zeros(4), good)
    _merge_close(before, scale0, ref, ref_scale)
    for k, bad in enumerate(([float("nan"), 1.0, 40.0], [1.0, float("inf"), 40.0], [float("-inf"), float("nan"), 40.0])):
        scale = ops.return_norm_merge(state, torch.tensor(bad, **f64))
        after = state.cpu().numpy()
        assert np.array_equal(after[:3], before[:3]) and after[3] == k + 1.0 and scale.item() == scale0


# ------------------------------------------------------------------------------------------------ 4: scale
@pytest.mark.parametrize("n", [1, 255, 1025])
@pytest.mark.parametrize("clip", [10.0, 0.0])
def test_scale_is_numpys_f32_product_and_clip_bit_for_bit(ops, n, clip):
    rng = np.random.default_rng(n)
    rew = (rng.standard_normal(n) * 40.0).astype(np.float32)
    if n > 4:
        rew[3] = np.nan
        rew[4] = np.inf
    sc = np.float32(0.37123)
    want = rew * sc
    if clip > 0:
        want = np.clip(want, np.float32(-clip), np.float32(clip))
    r = dev(rew)
    out = ops.reward_scale(r, dev(np.array([sc])), clip)
    got, ok = out.cpu().numpy(), ~np.isnan(want)         # a NaN is a NaN whatever its payload; every other value bit for bit
    assert want.dtype == np.float32 and out.dtype == torch.float32
    assert np.array_equal(np.isnan(got), ~ok) and np.array_equal(got[ok].view(np.uint32), want[ok].view(np.uint32))
    assert np.array_equal(r.cpu().numpy(), rew, equal_nan=True)                          # the input stays
    if n > 4:
        assert np.isnan(got[3]) and got[4] == (clip if clip > 0 else np.inf)
        assert clip == 0 or (np.abs(got[ok]) == clip).sum() > 1
    aliased = ops.reward_scale(r, dev(np.array([sc])), clip, out=r)
    assert aliased.data_ptr() == r.data_ptr() and np.array_equal(aliased.cpu().numpy(), got, equal_nan=True)


# ------------------------------------------------------------------------------------------------ 5: trainer
def _host_replay(replay, rew, done, gamma, clip, eps=1e-8):
    """One rollout through return_traces + merge_running, continuing `replay` = {state, carry}; returns the f32 scaled reward."""
    from uavppo.reward_norm import batch_stats, merge_running, return_traces
    G, replay["carry"] = return_traces(rew, done, gamma, replay["carry"])
    replay["state"], scale = merge_running(replay["state"], batch_stats(G), eps)
    return np.clip(rew * scale, np.float32(-clip), np.float32(clip)), scale


def _ulps(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    assert np.array_equal(np.signbit(a), np.signbit(b)) or np.abs(a - b).max() < 1e-30
    return int(np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64)).max())


@pytest.mark.parametrize("kind,hidden", [("mlp", 128), ("lstm", 64)])
def test_trainer_normalises_what_the_gae_reads_and_nothing_else(ops, kind, hidden):
    from uavppo.trainer import VecPPOTrainer
    tr = VecPPOTrainer(8, 16, policy=kind, hidden=hidden, device=DEV, seed=3, normalise_rewards=True)
    tr.radius = 200.0                       # episodes end inside the 16-step rollouts
    tr.reset()
    assert tr.reward_norm.state.cpu().tolist() == [0.0] * 4 and tr.reward_norm.gamma == tr.hp["gamma"] and tr.reward_norm.clip == 10.0
    replay = {"state": np.zeros(4), "carry": np.zeros(8)}
    for it in range(3):
        tr.collect()
        rew0, done = tr.buf["rew"].clone(), tr.buf["done"].cpu().numpy()
        tr.update()                         # its compute_advantages() is the rollout's one pass through the normaliser
        rn = tr.reward_norm.rew_n
        adv = ops.gae(rn, tr.buf["val"], tr.buf["done"], tr.hp["gamma"], tr.hp["lam"], tr.gae_mode, last_val=tr.last_val)
        assert torch.equal(tr.adv.view(torch.int32), adv.view(torch.int32))
        want, scale = _host_replay(replay, rew0.cpu().numpy(), done, tr.hp["gamma"], 10.0)
        assert _ulps(rn.cpu().numpy(), want) <= 2, it
        assert _ulp32(tr.reward_norm.host_scale(), scale) <= 1 and scale != 1.0
        assert torch.equal(tr.buf["rew"].view(torch.int32), rew0.view(torch.int32))
        tr.iteration += 1
    tr.losses()                             # raises on NaN
    assert tr.reward_norm.state[2].item() == 3.0 * 8 * 16 and tr.reward_norm.state[3].item() == 0.0
    tr.reset()
    assert tr.reward_norm.state.cpu().tolist() == [0.0] * 4 and tr.reward_norm.carry.abs().max().item() == 0.0
    assert tr.reward_norm.host_scale() == 1.0


@pytest.mark.parametrize("kind,hidden", [("mlp", 128), ("lstm", 64)])
def test_option_off_is_the_trainer_without_the_keyword(kind, hidden):
    from uavppo.trainer import VecPPOTrainer
    a = VecPPOTrainer(8, 16, policy=kind, hidden=hidden, device=DEV, seed=4)
    b = VecPPOTrainer(8, 16, policy=kind, hidden=hidden, device=DEV, seed=4, normalise_rewards=False)
    assert b.reward_norm is None
    for _ in range(3):
        a.train_iteration()
        b.train_iteration()
    assert torch.equal(a.policy.flat.view(torch.int32), b.policy.flat.view(torch.int32))
    assert torch.equal(a.exp_avg_sq.view(torch.int32), b.exp_avg_sq.view(torch.int32))


_CHILD = """
import hashlib, json, sys
sys.path[:0] = [%r, %r]
import torch
from uavppo.dist_utils import collectives_on, use_abi_collectives
from uavppo.trainer import VecPPOTrainer
use_abi_collectives(0, 1, "cuda:0")
assert collectives_on()
tr = VecPPOTrainer(8, 16, policy="lstm", hidden=64, device="cuda:0", seed=8, normalise_rewards=True)
for _ in range(2):
    tr.train_iteration()
tr.losses()
sha = lambda t: hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()
print(json.dumps({"flat": sha(tr.policy.flat), "rew_n": sha(tr.reward_norm.rew_n), "state": tr.reward_norm.state.cpu().tolist(),
                  "scale": tr.reward_norm.host_scale()}))
"""


def test_the_all_reduce_of_the_batch_sums_on_a_one_rank_communicator_changes_nothing():
    """The normaliser's exchange issued for real: a one-rank RCCL communicator on the C ABI's carrier with UAVPPO_FORCE_COLLECTIVES=1
    (the carrier is process-wide state, hence a child process), against the same job here, without collectives.  A sum over one
    rank changes nothing: the same bits."""
    import hashlib
    import json
    import os
    import subprocess
    import sys
    from uavppo.trainer import VecPPOTrainer
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = _CHILD % (root, os.path.join(root, "uav-wrf-les-ppo-lstm_amd"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120, env=dict(os.environ, UAVPPO_FORCE_COLLECTIVES="1"))
    assert r.returncode == 0, r.stderr[-2000:]
    abi = json.loads(r.stdout.strip().splitlines()[-1])
    tr = VecPPOTrainer(8, 16, policy="lstm", hidden=64, device=DEV, seed=8, normalise_rewards=True)
    for _ in range(2):
        tr.train_iteration()
    tr.losses()
    sha = lambda t: hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()
    plain = {"flat": sha(tr.policy.flat), "rew_n": sha(tr.reward_norm.rew_n), "state": tr.reward_norm.state.cpu().tolist(),
             "scale": tr.reward_norm.host_scale()}
    assert plain == abi and plain["state"][2] == 2.0 * 8 * 16 and plain["scale"] != 1.0


# ------------------------------------------------------------------------------------------------ 6: GAIL
def test_gail_normalises_its_shaped_reward_and_leaves_it_unwritten(ops):
    from uavppo.gail import GAILTrainer
    rng = np.random.RandomState(31)
    expert = (rng.rand(200, 6).astype(np.float32), rng.randint(0, 5, 200).astype(np.int64))
    tr = GAILTrainer(8, 16, "mlp", device=DEV, seed=5, use_curriculum=False, expert=expert, gail_coef=0.5, env_coef=0.75,
                     normalise_rewards=True, reward_clip=2.0)
    tr.disc.flat.mul_(3.0)
    for _ in range(2):
        tr.collect()
        rew0 = tr.buf["rew"].clone()
        tr.update()
        shaped = ops.disc_reward(tr.disc.flat, *tr._rows(), tr.n_act, 0.5, 0.75, rew_env=tr.buf["rew"].view(-1)).view(8, 16)
        assert torch.equal(tr.rew_shaped.view(torch.int32), shaped.view(torch.int32)) and not torch.equal(shaped, rew0)
        assert torch.equal(tr.buf["rew"].view(torch.int32), rew0.view(torch.int32))
        sc = np.float32(tr.reward_norm.host_scale())
        want = np.clip(shaped.cpu().numpy() * sc, np.float32(-2.0), np.float32(2.0))
        assert sc != 1.0 and np.array_equal(tr.reward_norm.rew_n.cpu().numpy().view(np.uint32), want.view(np.uint32))
        adv = ops.gae(tr.reward_norm.rew_n, tr.buf["val"], tr.buf["done"], tr.hp["gamma"], tr.hp["lam"], tr.gae_mode)
        assert torch.equal(tr.adv.view(torch.int32), adv.view(torch.int32))
        tr._after_update()                  # the discriminator step: the next rollout's shaped reward is on another scale
        tr.iteration += 1


# ------------------------------------------------------------------------------------------------ 7: state_dict
def test_state_dict_round_trip_reproduces_rew_n_bit_for_bit():
    from uavppo.trainer import VecPPOTrainer
    a = VecPPOTrainer(8, 16, policy="mlp", device=DEV, seed=6, normalise_rewards=True)
    a.radius = 200.0
    a.reset()
    for _ in range(2):
        a.train_iteration()
    sd = a.reward_norm.state_dict()
    assert sorted(sd) == ["carry", "state"] and all(isinstance(v, np.ndarray) and v.dtype == np.float64 for v in sd.values())
    assert sd["state"].shape == (4,) and sd["carry"].shape == (8,) and sd["state"][2] == 2.0 * 8 * 16
    b = VecPPOTrainer(8, 16, policy="mlp", device=DEV, seed=99, normalise_rewards=True)
    b.reward_norm.load_state_dict(sd)
    assert _ulp32(b.reward_norm.host_scale(), a.reward_norm.host_scale()) <= 1      # restated on the host; the next merge writes it again
    a.collect()
    for k in ("rew", "done", "val"):
        b.buf[k].copy_(a.buf[k])
    a.compute_advantages()
    b.compute_advantages()
    assert torch.equal(a.reward_norm.rew_n.view(torch.int32), b.reward_norm.rew_n.view(torch.int32))
    assert torch.equal(a.reward_norm.state, b.reward_norm.state) and torch.equal(a.reward_norm.carry, b.reward_norm.carry)
    assert torch.equal(a.adv.view(torch.int32), b.adv.view(torch.int32))
    with pytest.raises(ValueError):
        b.reward_norm.load_state_dict({"state": sd["state"], "carry": sd["carry"][:3]})
